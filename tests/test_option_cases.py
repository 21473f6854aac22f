"""tests/_option_cases.py against the code, without a GPU: the table lists the entry points that read a launch option (found in
x266_amd/csrc/x266hip_abi.hip itself), its values are the ones kOptions accepts, the Python clamp is units_per_wave_for compiled from
x266_device.hpp, the shapes of every row meet the coverage conditions, and no setting that names a loop runs the default loop only."""
import os
import re
import subprocess

import _cpp_driver
import _option_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "x266_amd", "csrc")

# entry points that reach an option without launching under it: the option calls themselves, the autotuner's report, and the timing
# probe, which repeats launch_op on the caller's buffers
NOT_ROWS = {"xHipSetOption", "xHipGetOption", "xHipAutotuneReport", "xHipTimeKernel"}
KEYWORDS = {"if", "for", "while", "switch", "catch", "return", "sizeof", "static_assert", "defined"}


def _code(text):
    """the source without comments, string literals and preprocessor lines"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)


def function_bodies(text):
    """{name: body} of the functions defined in the source, lambdas and nested blocks inside their function; namespaces, extern blocks
    and structs are walked through (a member function counts as a function)"""
    code, out, pos = _code(text), {}, 0
    head = re.compile(r"\b([A-Za-z_]\w*)\s*\(")
    while True:
        m = head.search(code, pos)
        if not m:
            return out
        depth, i = 1, m.end()
        while i < len(code) and depth:                                          # the matching parenthesis
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            i += 1
        after = re.match(r"\s*(?:const\s*)?\{", code[i:])
        if m.group(1) in KEYWORDS or not after:
            pos = m.end()
            continue
        start = i + after.end()
        depth, j = 1, start
        while j < len(code) and depth:
            depth += {"{": 1, "}": -1}.get(code[j], 0)
            j += 1
        out[m.group(1)] = out.get(m.group(1), "") + code[start:j - 1]
        pos = j


def k_options(text):
    """{key: (member, lo, hi, multiple_of)} of kOptions, "autotune" (whose upper bound is an expression) left out"""
    table = re.search(r"static const OptionDesc kOptions\[\] = \{(.*?)\n\};", text, re.S).group(1)
    rows = re.findall(r'\{"(\w+)", &x266hip_ctx::(\w+), (\d+), ([^,]+), (\d+)\}', table)
    assert len(rows) == 13 and "autotune" in [r[0] for r in rows], rows
    return {key: (member, int(lo), int(hi), int(mult)) for key, member, lo, hi, mult in rows if key != "autotune"}


def option_readers(text):
    """{function: set of option keys} for the functions of the source that read an option through ctx-> themselves or call one that does"""
    bodies, members = function_bodies(text), {member: key for key, (member, _, _, _) in k_options(text).items()}
    reads = {f: {members[m] for m in re.findall(r"\bctx->(\w+)\b", body) if m in members} for f, body in bodies.items()}
    calls = {f: {g for g in bodies if g != f and re.search(r"\b%s\s*\(" % g, body)} for f, body in bodies.items()}
    changed = True
    while changed:
        changed = False
        for f in bodies:
            more = set().union(*[reads[g] for g in calls[f]]) - reads[f] if calls[f] else set()
            if more:
                reads[f] |= more
                changed = True
    return {f: r for f, r in reads.items() if r}


def _abi(root=ROOT):
    return open(os.path.join(root, "x266_amd", "csrc", "x266hip_abi.hip")).read()


def entry_points_reading_options(text):
    return {f for f in option_readers(text) if re.fullmatch(r"x[A-Z]\w*", f)} - NOT_ROWS


def check_table_against(text, rows):
    """the assertion of test_the_table_lists_what_the_code_reads, on any source text and any set of rows (the mutation checks of the
    table use it on changed copies)"""
    found, listed = entry_points_reading_options(text), {r.entry for r in rows.values()}
    assert found == listed, ("read an option, no row: %s; a row, read no option: %s" % (sorted(found - listed), sorted(listed - found)))


def test_the_parser_finds_the_helpers():
    readers = option_readers(_abi())
    for helper in ("cfg_for", "launch_op", "inv_to_tiles_cfg", "ctu_tiles_cfg", "satd_search_call", "host_batch"):
        assert helper in readers, helper
    assert "me_tile_rows" in readers["satd_search_call"] and "adaptive_per_wave" in readers["host_batch"]
    assert "xSadBatchDev" not in readers and "xDct32PassDev" not in readers       # "autotune" alone, and no option at all


def test_the_table_lists_what_the_code_reads():
    text = _abi()
    check_table_against(text, oc.ROWS)
    readers, options = option_readers(text), k_options(text)
    for row in oc.ROWS.values():
        assert set(row.options) | set(row.unused) | set(row.base) <= readers[row.entry], row.name
        assert set(row.base) <= set(options) and not set(row.base) & set(oc.swept(row)), row.name
    assert set(options) == set(oc.VALUES) == set(oc.DEFAULTS)
    assert set(options) == set().union(*[set(r.options) for r in oc.ROWS.values()])             # every option reaches some launch


def test_a_row_taken_out_or_a_reader_added_fails():
    """the check above is tied to both sides: without a row, and with cfg_for in an entry point that has none, it fails"""
    text = _abi()
    fewer = {k: r for k, r in oc.ROWS.items() if r.entry != "xDct32InvCtuToTilesDev"}
    try:
        check_table_against(text, fewer)
    except AssertionError as e:
        assert "xDct32InvCtuToTilesDev" in str(e)
    else:
        raise AssertionError("a missing row went unnoticed")
    head = "    return launched(ctx, \"1-D pass launch\""
    assert text.count(head) == 1
    try:
        check_table_against(text.replace(head, "    (void)cfg_for(ctx, 0);\n" + head), oc.ROWS)
    except AssertionError as e:
        assert "xDct32PassDev" in str(e)
    else:
        raise AssertionError("a new reader went unnoticed")


def test_the_values_are_the_ones_the_library_accepts():
    options = k_options(_abi())
    for key, (member, lo, hi, mult) in options.items():
        for v in oc.VALUES[key]:
            assert lo <= v <= hi and v % mult == 0, (key, v)
        assert lo <= oc.DEFAULTS[key] <= hi and oc.DEFAULTS[key] in oc.VALUES[key], key
        default = re.search(r"\b%s = (\d+)" % member, _abi())
        assert default and int(default.group(1)) == oc.DEFAULTS[key], key                 # the context's initialiser
    for key in oc.PER_WAVE:
        assert {options[key][1], options[key][2], 2, 3, 9} <= set(oc.VALUES[key]), key
    for key in oc.WG_OPTIONS:
        assert set(oc.VALUES[key]) == {0, 64, 128, 192, 256} and options[key][1:] == (0, 256, 64), key
    assert set(oc.PER_WAVE) == {k for k in options if k.endswith("_per_wave") and k not in ("adaptive_per_wave", "satd_lds_bytes_per_wave")}
    assert oc.VALUES["me_tile_rows"] == tuple(range(options["me_tile_rows"][1], options["me_tile_rows"][2] + 1))
    assert oc.VALUES["tile_tiles_per_wave"] == (0, 1, 2, 3, 9, 64) and oc.VALUES["satd_lds_bytes_per_wave"] == (0, 16, 4096, 6144, 9216, 16384)


def test_every_setting_rule_is_applied():
    for row in oc.ROWS.values():
        sets = oc.settings(row)
        assert all(set(s) <= set(oc.swept(row)) | set(row.base) for s in sets), row.name
        assert all(all(s[k] == v for k, v in row.base.items()) for s in sets), row.name
        for o in oc.swept(row):
            for v in oc.VALUES[o]:
                assert any(s.get(o, oc.DEFAULTS[o]) == v and all(s[k] == oc.DEFAULTS[k] for k in s if k not in (o, oc.ADAPTIVE) and k not in row.base)
                           for s in sets), (row.name, o, v)
        for s in sets:                                                            # a per-wave value off its default: adaptive 0, but for the clamp's own settings
            for o in oc.PER_WAVE:
                if s.get(o, oc.DEFAULTS[o]) != oc.DEFAULTS[o] and oc.ADAPTIVE in oc.swept(row) and s.get(oc.ADAPTIVE, 1):
                    assert s[o] == 9 or all(s[k] == max(oc.VALUES[k]) for k in oc.swept(row)), (row.name, s)
        if row.loop and row.pairs:
            for wg in oc.VALUES[row.wg] if row.wg else ():
                for v in oc.VALUES[row.loop]:
                    assert any(s.get(row.wg) == wg and s.get(row.loop) == v and s.get(oc.ADAPTIVE) == 0 for s in sets), (row.name, wg, v)
            assert any(s.get(row.loop) == 9 and s.get(oc.ADAPTIVE) == 1 for s in sets), row.name
        assert any(all(s.get(k) == max(oc.VALUES[k]) for k in oc.swept(row)) for s in sets), row.name


def _cut(text, start):
    """the declaration that begins with `start`, up to the brace that closes it"""
    at = text.index(start)
    depth, i = 0, text.index("{", at)
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
        if depth == 0:
            return text[at:i]


GRID_OPTIONS = list(range(11)) + [4096]
GRID_UNITS = sorted(set(list(range(0, 64)) + list(range(64, 50001, 97)) + [2559, 2560, 2561, 10239, 10240, 20479, 20480, 20481, 24320, 40960, 50000]))
GRID_CUS = (64, 256, 304)


@_cpp_driver.needs_gxx
def test_the_python_clamp_is_the_librarys(tmp_path):
    hpp = open(os.path.join(CSRC, "x266_device.hpp")).read()
    cfg, rule = _cut(hpp, "struct LaunchCfg {") + ";", _cut(hpp, "inline unsigned units_per_wave_for(")
    main = """
int main()
{
    const int options[] = {%s};
    const size_t units[] = {%s};
    const int cus[] = {%s};
    for (int cu : cus) for (int adaptive = 0; adaptive < 2; ++adaptive) for (int o : options) for (size_t n : units) {
        LaunchCfg c = {cu, adaptive, o, 64, 0, 0};
        std::printf("%%u\\n", units_per_wave_for(c, n));
    }
    return 0;
}
""" % (", ".join(map(str, GRID_OPTIONS)), ", ".join(map(str, GRID_UNITS)), ", ".join(map(str, GRID_CUS)))
    src = tmp_path / "clamp.cpp"
    src.write_text("#include <cstddef>\n#include <cstdio>\n" + cfg + "\n" + rule + "\n" + main)
    exe, r = _cpp_driver.build(tmp_path, "clamp", source=src)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(x) for x in out.stdout.split()]
    want = [oc.per_wave_in_force(o, n, adaptive, cu) for cu in GRID_CUS for adaptive in (0, 1) for o in GRID_OPTIONS for n in GRID_UNITS]
    assert got == want
    assert oc.per_wave_in_force(9, 20479, 1, 256) == 1 and oc.per_wave_in_force(9, 20480, 1, 256) == 2 and oc.per_wave_in_force(9, 20479, 0, 256) == 9


def test_the_satd_launchers_defaults():
    """0 groups per wave = 2 for the staged body and the frame lanes, 4 for the LDS-DMA body: the launchers say so themselves"""
    src = open(os.path.join(CSRC, "satd_kernels.hip")).read()
    assert "if (c.units_per_wave <= 0) c.units_per_wave = dma ? 4 : 2;" in src and "if (c.units_per_wave <= 0) c.units_per_wave = 2;" in src
    assert "constexpr size_t kSatdDmaMinBlocks = (size_t)3 << 20;" in open(os.path.join(CSRC, "x266_device.hpp")).read()
    assert [oc.satd_default_groups(v, 1000) for v in (0, 1, 3)] == [2, 2, 4]
    assert oc.satd_default_groups(0, oc.SATD_DMA_MIN_BLOCKS) == 4 and oc.satd_default_groups(3, 1000, frame_lanes=True) == 2


def test_the_shapes_meet_the_conditions():
    for row in oc.ROWS.values():
        assert oc.missing(row) == [], row.name
        assert len({tuple(sorted((k, str(v)) for k, v in s.items())) for s in row.shapes}) == len(row.shapes), row.name
        assert max(row.units(s) for s in row.shapes) < 4096, row.name            # "a few thousand units"
    cut = [s["size"] for s in oc.ROWS["xTransformCtuToTilesDev"].shapes]
    assert (80, 48) in cut and (208, 144) in cut and any(w % 64 and h % 64 for w, h in cut)
    assert oc.ROWS["xTransformCtuFromTilesDev"].shapes == oc.ROWS["xTransformCtuToTilesDev"].shapes


def test_the_conditions_notice_a_missing_shape():
    row = oc.ROWS["xDct32InvCtuToTilesDev"]
    assert oc.missing(row._replace(shapes=[s for s in row.shapes if s["size"] != (128, 64)])) == ["waves % 3 == 1"]
    row = oc.ROWS["xDct32InvToTilesDev"]
    assert "per-wave 9: p * W * k" in oc.missing(row._replace(shapes=[s for s in row.shapes if s["size"] != (192, 96)]))


def test_no_setting_runs_the_default_loop_only():
    """the vacuity check: a setting that names a per-wave value above 1 with "adaptive_per_wave" 0 runs that many units per wave on some
    shape of its row whose last run is short -- and with "adaptive_per_wave" left at 1 it would run one (what the repaired tests ran)"""
    checked = 0
    for row in oc.ROWS.values():
        for s in oc.settings(row):
            if not row.loop or s.get(oc.ADAPTIVE, 1):
                continue
            live = [sh for sh in row.shapes if row.live(sh)]
            value = s.get(row.loop, oc.DEFAULTS[row.loop])
            if (value or min(row.zero(s, sh) for sh in live)) <= 1:
                continue
            hit = [sh for sh in live if oc.loop_length(row, s, sh) == oc.intended_length(row, s, sh) == (value or row.zero(s, sh))
                   and oc.short_last_run(row.units(sh), oc.loop_length(row, s, sh))]
            assert hit, (row.name, s)
            assert all(oc.loop_length(row, dict(s, **{oc.ADAPTIVE: 1}), sh) == 1 for sh in live), row.name
            checked += 1
    assert checked > 300


def test_the_header_names_the_calls_of_every_option():
    """include/x266hip.h lists, per option, the entry points of the table's rows that the option reaches"""
    hdr = open(os.path.join(ROOT, "include", "x266hip.h")).read()
    block = hdr[hdr.index("The calls that take each option"):hdr.index("Rounds 1-3 had")]
    stated = {key: set(re.findall(r"\bx[A-Z]\w+", text)) for key, text in re.findall(r'"(\w+)":(.*?)(?=\n \*   "|\Z)', block, re.S)}
    want = {key: {r.entry for r in oc.ROWS.values() if key in r.options or key in r.base} for key in oc.DEFAULTS}
    per_wave = set().union(*[want[key] for key in oc.PER_WAVE])
    assert want.pop(oc.ADAPTIVE) == per_wave and not stated.pop(oc.ADAPTIVE)            # "every call above that takes a per-wave option"
    assert stated == want, {k: (sorted(stated.get(k, set()) - want[k]), sorted(want[k] - stated.get(k, set()))) for k in want if stated.get(k) != want[k]}
    assert "CU count x 40 x 2" in hdr[hdr.index("Launch options"):hdr.index("The calls that take each option")]
