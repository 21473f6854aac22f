"""CPU: the surface and the argument rules of xEntropyEncodeLevelsGpu and xEntropyDecodeLevelsGpu: header, struct layout, exports, bindings,
and the rule functions of x266_amd/csrc/x266_args.hpp (entropy_encode, entropy_decode) against the contract as
tests/cpp/entropy_rules_check.cpp writes it down -- single perturbations of a base tuple: alignment halves, saturating extents, every illegal
overlap, a NULL d_stream with a non-zero capacity, an entry of init at 30 and at 2018.  The same driver runs the host coder of
x266_amd/csrc/x266_entropy.hpp against literals that this file prints from tests/_entropy_ref.py (python tests/test_entropy_arg_rules.py),
and this file holds those literals against the reference as it stands.  The driver is a stand-alone program, built twice: plain, and with
the address and undefined-behaviour sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _cpp_driver
import _entropy_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xEntropyEncodeLevelsGpu", "xEntropyDecodeLevelsGpu")
HELPERS = ("xEntropyDefaultInit", "xEntropyEncodeRegion", "xEntropyDecodeRegion")
DRIVER = "entropy_rules_check"
CHECK_FLOOR = 1500                                                        # a walk that shrank must not pass quietly
CASES = [(3, 0, 0), (0, 0, 0), (3, 0, 5), (2, 0, 6), (1, 0, 7), (0, 0, 8), (3, 2, 40), (2, 2, 77), (1, 2, 114), (0, 2, 36), (3, 0, 73), (0, 1, 1), (1, 1, 1), (2, 1, 1),
         (3, 1, 1), (3, 0, 2)]                                             # (k, table, seed)


def case_levels(seed):
    """the driver's recipe, restated"""
    x, density, out = seed, seed % 37 + 1, []
    for i in range(1024):
        x = (x * 1103515245 + 12345) & 0xFFFFFFFF
        l = 0
        if seed == 1:
            l = -32767 if i % 3 == 0 else 32767
        elif seed != 0 and (x >> 16) % 97 < density:
            l = ((x >> 9) % 65535) - 32767 if (x >> 8) % 7 == 0 else ((x >> 20) % 9) - 4
            l = l or 1
        out.append(l)
    return np.array(out, np.int16)


def case_table(kind):
    return None if kind == 0 else E.worst_init() if kind == 1 else np.array([31 + (i * 1986) // 99 for i in range(E.CONTEXTS)], np.uint16)


def literals():
    """{table: rows of integers}: what tests/cpp/entropy_rules_check.cpp holds x266_entropy.hpp against"""
    cases, rows = [], []
    for k, kind, seed in CASES:
        lv = case_levels(seed)
        data, ctx, byp = E.encode_region(lv, k, case_table(kind))
        cases.append([k, kind, seed, int(np.count_nonzero(lv)), ctx, byp, len(data), len(rows)])
        rows.append([data[i] if i < len(data) else -1 for i in range(24)] + [sum(data)])
    return {"CASE": cases, "BYTES": rows}


def source_tables():
    src = open(os.path.join(ROOT, "tests", "cpp", DRIVER + ".cpp")).read()
    got = {}
    for name, body in re.findall(r"static const int (\w+)\[\d+\]\[\d+\] = \{(.*?)\};", src, re.S):
        got[name] = [[int(v.strip()) for v in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]
    return got


def test_the_drivers_literals_are_the_references():
    want, got = literals(), source_tables()
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name
    assert {row[0] for row in want["CASE"]} == {0, 1, 2, 3} and {row[1] for row in want["CASE"]} == {0, 1, 2}
    assert any(row[6] == 0 for row in want["CASE"]) and max(row[6] for row in want["CASE"]) > 4000                # an empty and a maximal substream
    assert any(int(np.abs(case_levels(row[2]).astype(np.int64)).max()) > 20000 for row in want["CASE"])         # the long remainders


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="entropy_rules_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared coder compiles without a warning as plain C++
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
    assert int(re.search(r"^checks x266_entropy_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR
    assert "sizeof(x266_entropy_region_t) 32" in text and "sizeof(x266_entropy_t) 72" in text


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment; the driver's
    line of each call names fields of the struct in struct order at that alignment, optional where the comment says "or NULL" """
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    stated = _cpp_driver.header_struct_fields("x266_entropy_t")
    assert list(stated) == ["d_level", "d_class", "d_nnz", "d_region", "d_stream", "d_total"]
    assert {f: v[0] for f, v in stated.items()} == {"d_level": 16, "d_class": 1, "d_nnz": 4, "d_region": 8, "d_stream": 16, "d_total": 8}
    for call in CALLS:
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_entropy_t \*p, void \*stream\);" % call, hdr)
        held = driver_fields(call)
        assert list(held) == [f for f in stated if f in held]
        for field, (align, optional, _) in held.items():
            assert align == stated[field][0] and optional == stated[field][1], (call, field)
    assert list(driver_fields(CALLS[0])) == list(stated) and list(driver_fields(CALLS[1])) == list(stated)[:5]
    assert {f for f, v in driver_fields(CALLS[0]).items() if v[2]} == {"d_region", "d_stream", "d_total"}
    assert {f for f, v in driver_fields(CALLS[1]).items() if v[2]} == {"d_level", "d_nnz"}
    body = re.search(r"typedef struct x266_entropy_region_t \{(.*?)\} x266_entropy_region_t;", hdr, re.S).group(1)
    assert re.findall(r"\buint(?:32|64)_t\s+(\w+);", body) == ["ctx_bins", "bypass_bins", "offset", "n_words", "n_bytes", "n_nz", "reserved"]
    assert re.search(r"const uint16_t \*init;\s*/\* HOST memory", hdr)
    text = hdr[hdr.index("---- the entropy coder"):hdr.index("typedef struct x266_entropy_region_t")]
    for said in ("cbf", "cgf", "gt1", "gt2", "Exp-Golomb", "-32768", "cannot leave the block", "31 .. 2017", "0xFFFFFFFF", "0xFFFFFF", "Worked values",
                 "X266_ENTROPY_MAX_BYTES", "count-only", "Malformed", "longer than 14", "+32768", "Out of scope", "motion stream", "carry-over", "Sign hiding".lower(),
                 "dependent quantisation", "residual's alone"):
        assert said in text, said


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    import x266_amd.entropy as X
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + HELPERS:
        assert name in exported and hasattr(lib, name), name
    assert not [n for n in exported if "entropy" in n.lower() and not n.startswith("xEntropy")]     # internal C++ symbols stay local
    for call in CALLS:
        fn = getattr(lib, call)
        assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.EntropyParams)
        p = X.entropy_params(d_level=0x1000, d_region=0x3000, init=0x5000, n_regions=7, cap_words=5)
        assert (p.d_level, p.d_class, p.d_nnz, p.d_region, p.d_stream, p.d_total, p.init, p.n_regions, p.cap_words) == (0x1000, None, None, 0x3000, None, None, 0x5000, 7, 5)
        assert fn(None, ctypes.byref(p), None) == -1                          # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1                                     # ... and so is a NULL p
    assert ctypes.sizeof(x266_amd.EntropyParams) == 72 and x266_amd.EntropyParams.init.offset == 48 and x266_amd.EntropyParams.cap_words.offset == 64
    assert x266_amd.ENTROPY_REGION_DTYPE.itemsize == 32 and x266_amd.ENTROPY_REGION_DTYPE == E.RECORD_DTYPE


def test_the_binding_and_the_one_copy_of_the_coder():
    """entropy_params refuses an unknown field in the keyword builders' words; the numpy calls are module functions, and the Codec gains the
    two ..._dev methods.  The kernels, the rules and the host helpers take the coder from x266_entropy.hpp; the offset scan is one kernel for
    the three streams"""
    import x266_amd
    import x266_amd.entropy as X
    with pytest.raises(TypeError) as e:
        X.entropy_params(bogus=1, d_level=16)
    assert str(e.value) == "entropy_params: no such field: ['bogus']"
    assert [n for n in dir(x266_amd.Codec) if "entropy" in n] == ["entropy_decode_levels_dev", "entropy_encode_levels_dev"]
    for name in ("entropy_params", "entropy_encode_levels", "entropy_decode_levels", "entropy_default_init", "entropy_encode_region", "entropy_decode_region"):
        assert callable(getattr(X, name)), name
    src = open(os.path.join(ROOT, "x266_amd", "entropy.py")).read()
    assert "codec._upload(" in src and "codec._fetch(" in src and "Codec._keyword_params(" in src       # the shared pieces, not copies
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, shared, levels_h, abi = (open(os.path.join(csrc, n)).read() for n in ("entropy_kernels.hip", "x266_entropy.hpp", "x266_levels.hpp", "x266hip_abi.hip"))
    assert '#include "x266_entropy.hpp"' in kernel and '#include "x266_entropy.hpp"' in abi
    for name in ("entropy_encode_region", "entropy_decode_region", "entropy_enc_finish", "entropy_dec_start"):
        assert re.search(r"inline \w+ %s\(" % name, shared) and name + "(" in kernel and name + "(" in abi, name
    assert len(re.findall(r"void levels_scan_kernel\(", levels_h)) == 1 and "void levels_scan_kernel" not in kernel
    assert "levels_scan_kernel<x266_entropy_region_t>" in kernel
    assert not re.search(r"atomic(Add|Min|Max|CAS|Exch)|__hip_atomic|while\s*\(", kernel)            # no atomics, no spin-wait
    assert not re.search(r"\bdo\b|while\s*\(\s*(1|true)\s*\)|for\s*\(\s*;\s*;", shared)                # bounded trip counts only
    assert kernel.count("hipLaunchKernelGGL(") == 4                                                # encode: count, scan, write; decode: one


if __name__ == "__main__":
    for name, rows in literals().items():
        print("static const int %s[%d][%d] = {%s};" % (name, len(rows), len(rows[0]), ", ".join("{%s}" % ", ".join(str(v) for v in row) for row in rows)))
