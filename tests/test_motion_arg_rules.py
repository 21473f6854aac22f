"""CPU: the surface and the argument rules of xMotionPackGpu and xMotionUnpackGpu: header, struct layout, exports, bindings, and the rule
functions of x266_amd/csrc/x266_args.hpp (motion_pack, motion_unpack) against the contract as tests/cpp/motion_rules_check.cpp writes it
down -- single perturbations of a base tuple: alignment halves, saturating extents, every illegal overlap, a NULL d_stream with a non-zero
capacity, sides that are no multiple of 16.  The same driver runs the arithmetic the kernels share with the host
(x266_amd/csrc/x266_motion.hpp) against literals that this file prints from tests/_motion_ref.py (python tests/test_motion_arg_rules.py), and
this file holds those literals against the reference as it stands.  The driver is a stand-alone program, built twice: plain, and with the
address and undefined-behaviour sanitizers.  g++ only: no GPU, no HIP."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _cpp_driver
import _motion_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("xMotionPackGpu", "xMotionUnpackGpu")
HELPERS = ("xMotionWalk", "xMotionPredictor", "xMotionVectorBits")
DRIVER = "motion_rules_check"
CHECK_FLOOR = 1200                                                        # a walk that shrank must not pass quietly
FIELD = [(57, 18), (-6, 90), (20000, -20000), (-60, -4), (-28, -27), (-15, 22), (6, -26), (32767, -32768), (24, 0), (72, 13), (-11, -78), (2, -22),
         (-45, -9), (-32768, 32767), (-20, 17), (21, 30), (6, 54), (19, -5), (87, 8), (-16, -63), (-3, -27), (-30, -14), (23, 3), (-25, 12)]
MASK_SHAPES = [(64, 64, 0, 2), (80, 48, 0, 2), (80, 48, 1, 2), (144, 112, 4, 2), (16, 16, 0, 2), (144, 112, 1, 259)]      # (width, height, CTU, seed of the tree)


# ---- the driver's literals, from the reference --------------------------------------------------------------------------------------------
def literals():
    """{table: rows of integers}: what tests/cpp/motion_rules_check.cpp holds x266_motion.hpp against"""
    t = {"FIELD": [list(v) for v in FIELD]}
    field = np.array(FIELD, np.int64).reshape(4, 6, 2)                      # 48 x 32: one CTU, cut on both sides
    t["PRED"] = [[k, nx << k, ny << k, *M.predictor(field, nx << k, ny << k, 1 << k)] for k in range(3) for ny in range(4 >> k) for nx in range(6 >> k)]
    t["MORTON"] = [[x, y, M.morton(x, y)] for x, y in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 1), (0, 2), (2, 2), (7, 0), (0, 7), (5, 3), (7, 7))]
    t["CRIGHT"] = [[bw, X, Y, n, int(M.predictor_spots(bw, 14, X, Y, n)[1] == "right")]
                   for bw, X, Y, n in ((4, 0, 2, 2), (4, 2, 2, 2), (4, 1, 1, 1), (18, 6, 8, 2), (18, 7, 8, 1), (18, 8, 8, 8), (18, 15, 9, 1), (18, 16, 8, 2), (18, 3, 0, 1), (18, 4, 4, 4),
                                       (18, 12, 4, 4), (18, 9, 1, 1), (18, 8, 1, 1), (18, 17, 3, 1))]
    masks, heads, walks = [], [], []
    rs = np.random.RandomState(4)
    for w, h, c, seed in MASK_SHAPES:
        bw, bh, cw, ch = M.grid(w, h)
        mv, level = M.random_tree(w, h, seed)
        r = M.pack(mv, level, w, h)
        good = int(r["ctu"]["head_mask"][c])
        lev = level.reshape(bh, bw)
        for i in range(0, 64, 7):                                           # pack's walk from a block's side: the level bytes of its nodes' first blocks
            x, y = M.unmorton(i)
            X, Y = 8 * (c % cw) + x, 8 * (c // cw) + y
            if X < bw and Y < bh:
                lv = [int(lev[(Y >> k) << k, (X >> k) << k]) for k in (1, 2, 3)]
                walks.append([w, h, c, i, *lv, int(lev[Y, X])])
        for mask in [good, good & ~1, good | 1 << 63, 0b101, 1] + [good ^ (1 << int(rs.randint(64))) for _ in range(4)]:
            ok = M.well_formed(bw, bh, c % cw, c // cw, mask)
            hs = [i for i in range(64) if (mask >> i) & 1] if ok else []
            masks.append([w, h, c, mask, len(hs)])
            heads += [[len(masks) - 1, j, i, M.level_from_mask(bw, bh, c % cw, c // cw, mask, i)] for j, i in enumerate(hs)]
    t["MASK"], t["HEAD"], t["WALK"] = masks, heads, walks
    bits = []
    for w, h, seed in ((144, 112, 259), (80, 48, 3)):
        mv, level = M.random_tree(w, h, seed)
        r = M.pack(mv, level, w, h)
        for c in range(len(r["ctu"])):
            bits.append([w, h, c, int(r["ctu"]["parts"][c]), int(r["ctu"]["bits"][c]), int(r["ctu"]["max_abs"][c])])
    t["BITS"] = bits
    return t


def source_tables():
    src = open(os.path.join(ROOT, "tests", "cpp", DRIVER + ".cpp")).read()
    got = {}
    for name, body in re.findall(r"static const (?:int|unsigned long long) (\w+)\[\d+\]\[\d+\] = \{(.*?)\};", src, re.S):
        got[name] = [[int(v.strip().rstrip("ULL")) for v in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]
    return got


def test_the_drivers_literals_are_the_references():
    want, got = literals(), source_tables()
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name
    assert any(row[4] == 0 for row in want["MASK"]) and any(row[4] > 1 for row in want["MASK"])     # malformed and well-formed masks
    assert {row[3] for row in want["HEAD"]} == {0, 1, 2, 3} and {row[7] for row in want["WALK"]} == {0, 1, 2, 3}
    assert {row[4] for row in want["CRIGHT"]} == {0, 1} and max(row[5] for row in want["BITS"]) == 65535


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def driver_output():
    with tempfile.TemporaryDirectory(prefix="motion_rules_") as where:
        exe, r = _cpp_driver.build(where, DRIVER)
        assert r.returncode == 0, r.stderr[-4000:]
        assert not r.stderr.strip(), r.stderr[-4000:]                        # the shared arithmetic compiles without a warning as plain C++
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
    assert int(re.search(r"^checks x266_motion_t (\d+)$", text, re.M).group(1)) >= CHECK_FLOOR
    assert "sizeof(x266_motion_ctu_t) 32" in text and "sizeof(x266_motion_t) 56" in text


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, DRIVER)


@_cpp_driver.needs_gxx
def test_the_header_declares_the_calls_and_the_driver_follows_its_comments():
    """context first, stream last, the device pointers in the struct; every pointer field's comment states its alignment; the driver's
    line of each call names fields of the struct in struct order at that alignment"""
    from test_gpu_placement import device_entry_points, header_alignments
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    stated = _cpp_driver.header_struct_fields("x266_motion_t")
    assert list(stated) == ["d_mv", "d_level", "d_ctu", "d_stream", "d_total"]
    assert {f: v[0] for f, v in stated.items()} == {"d_mv": 8, "d_level": 1, "d_ctu": 8, "d_stream": 16, "d_total": 8}
    for call in CALLS:
        assert call not in device_entry_points() and call not in header_alignments(every=True)   # the one table's parser must not count it
        assert re.search(r"int %s\s*\(x266hip_ctx \*ctx, const x266_motion_t \*p, void \*stream\);" % call, hdr)
        held = driver_fields(call)
        assert list(held) == [f for f in stated if f in held]
        for field, (align, optional, _) in held.items():
            assert align == stated[field][0] and not optional, (call, field)    # d_stream is optional only with cap_words == 0: the driver's walk
    assert list(driver_fields(CALLS[0])) == list(stated) and list(driver_fields(CALLS[1])) == list(stated)[:4]
    assert {f for f, v in driver_fields(CALLS[0]).items() if v[2]} == {"d_ctu", "d_stream", "d_total"}
    assert {f for f, v in driver_fields(CALLS[1]).items() if v[2]} == {"d_mv", "d_level"}
    body = re.search(r"typedef struct x266_motion_ctu_t \{(.*?)\} x266_motion_ctu_t;", hdr, re.S).group(1)
    assert re.findall(r"\buint(?:32|64)_t\s+(\w+);", body) == ["head_mask", "offset", "n_words", "parts", "bits", "max_abs"]
    region = re.search(r"typedef struct x266_level_region_t \{(.*?)\} x266_level_region_t;", hdr, re.S).group(1)
    assert re.findall(r"\b(uint(?:32|64)_t)\s+\w+;", body)[:3] == re.findall(r"\b(uint(?:32|64)_t)\s+\w+;", region)[:3]       # the first 20 bytes
    assert re.findall(r"\buint(?:32|64)_t\s+(\w+);", region)[1:3] == ["offset", "n_words"]
    text = hdr[hdr.index("compact motion stream"):hdr.index("typedef struct x266_motion_ctu_t")]
    for said in ("Morton", "0x1111", "canonicalises", "cannot be reproduced", "(int16_t)(P + (int16_t)word)", "Words 2 and 3", "untested", "Out of scope",
                 "count-only", "well formed"):
        assert said in text, said
    part = hdr[hdr.index("inter partition decision"):hdr.index("typedef struct x266_part_ctu_t")]
    assert "xMotionPackGpu" in part and "the motion side's compact stream" not in part
    assert "the motion side's compact stream is the follow-up" not in open(os.path.join(ROOT, "README.md")).read()


def test_the_library_exports_the_calls_and_they_refuse_null():
    import x266_amd
    import x266_amd.motion as X
    x266_amd.build_library()
    lib = x266_amd.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", x266_amd.lib_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in CALLS + HELPERS:
        assert name in exported and hasattr(lib, name), name
    assert not [n for n in exported if "motion" in n.lower() and not n.startswith("xMotion")]       # internal C++ symbols stay local
    for call in CALLS:
        fn = getattr(lib, call)
        assert fn.argtypes is not None and fn.argtypes[1] is ctypes.POINTER(x266_amd.MotionParams)
        p = X.motion_params(d_mv=0x1000, d_ctu=0x3000, width=144, height=112, cap_words=5)
        assert (p.d_mv, p.d_level, p.d_ctu, p.d_stream, p.d_total, p.width, p.height, p.cap_words) == (0x1000, None, 0x3000, None, None, 144, 112, 5)
        assert fn(None, ctypes.byref(p), None) == -1                          # a NULL context is refused, not dereferenced
        assert fn(None, None, None) == -1                                     # ... and so is a NULL p
    assert ctypes.sizeof(x266_amd.MotionParams) == 56 and x266_amd.MotionParams.width.offset == 40 and x266_amd.MotionParams.cap_words.offset == 48
    assert x266_amd.MOTION_CTU_DTYPE.itemsize == 32 and x266_amd.MOTION_CTU_DTYPE == M.CTU_DTYPE
    assert [x266_amd.MOTION_CTU_DTYPE.fields[n][1] for n in ("offset", "n_words")] == [x266_amd.LEVEL_REGION_DTYPE.fields[n][1] for n in ("offset", "n_words")]


def test_the_binding_and_the_one_copy_of_the_arithmetic():
    """motion_params refuses an unknown field in the keyword builders' words; the numpy calls are module functions, and the Codec gains the
    two ..._dev methods.  The kernels, the rules and the host helpers take the Morton map, the walk, the level-from-mask rule, the
    well-formedness test and the predictor from x266_motion.hpp, the geometry and the median from x266_part.hpp, L from x266_seed.hpp; the
    offset scan is one kernel for both streams"""
    import x266_amd
    import x266_amd.motion as X
    with pytest.raises(TypeError) as e:
        X.motion_params(bogus=1, d_mv=16)
    assert str(e.value) == "motion_params: no such field: ['bogus']"
    assert [n for n in dir(x266_amd.Codec) if "motion_pack" in n or "motion_unpack" in n] == ["motion_pack_dev", "motion_unpack_dev"]
    for name in ("motion_params", "motion_pack", "motion_unpack", "motion_walk", "motion_predictor", "motion_vector_bits"):
        assert callable(getattr(X, name)), name
    src = open(os.path.join(ROOT, "x266_amd", "motion.py")).read()
    assert "codec._upload(" in src and "codec._fetch(" in src and "Codec._keyword_params(" in src       # the shared pieces, not copies
    csrc = os.path.join(ROOT, "x266_amd", "csrc")
    kernel, rules, shared, part, levels, levels_h, abi = (open(os.path.join(csrc, n)).read() for n in
                                                          ("motion_kernels.hip", "x266_args.hpp", "x266_motion.hpp", "x266_part.hpp", "levels_kernels.hip",
                                                           "x266_levels.hpp", "x266hip_abi.hip"))
    assert '#include "x266_motion.hpp"' in kernel and '#include "x266_motion.hpp"' in abi and '#include "x266_part.hpp"' in shared
    for name in ("motion_part_level", "motion_predictor", "motion_block_covered", "motion_head_level", "motion_head_of", "motion_part_bits"):
        assert re.search(r"inline \w+ %s\(" % name, shared) and name + "(" in kernel, name
    for name in ("motion_mask_well_formed", "motion_head_level", "motion_predictor"):
        assert name + "(" in abi, name
    assert "part_predict3(" in shared and shared.count("part_median3") == 0 and part.count("part_predict3(") == 2      # defined once, used by part_predictor
    assert "seed_code_length(" in shared and "part_whole(" in shared                                  # L and the geometry have one copy
    assert len(re.findall(r"void levels_scan_kernel\(", levels_h)) == 1 and "void levels_scan_kernel" not in levels + kernel
    assert "levels_scan_kernel<x266_level_region_t>" in levels and "levels_scan_kernel<x266_motion_ctu_t>" in kernel
    assert not re.search(r"atomic(Add|Min|Max|CAS|Exch)|__hip_atomic|while\s*\(", kernel)            # no atomics, no spin-wait
    assert kernel.count("hipLaunchKernelGGL(") == 4                                                # pack: count, scan, write; unpack: one


if __name__ == "__main__":
    for name, rows in literals().items():
        kind = "unsigned long long" if name == "MASK" else "int"
        fmt = (lambda v: "%dULL" % v) if name == "MASK" else str
        print("static const %s %s[%d][%d] = {%s};" % (kind, name, len(rows), len(rows[0]), ", ".join("{%s}" % ", ".join(fmt(v) for v in row) for row in rows)))
