"""CPU: the cross-lane reductions and scans stand once, in x266_amd/csrc/x266_lanes.hpp, and the analysis kernels share one frame geometry.
Reads the sources only: no GPU, no compiler."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "x266_amd", "csrc")
LANES = "x266_lanes.hpp"
# a definition: the name after a return type, its parameter list, then the body's brace (a call is followed by `;`, `)` or an operator)
REDUCTION = re.compile(r"[\w>&*]\s+((?:wave_(?:sum|min|max|exclusive_sum)\w*|sum_over_\w+|shfl\w*64))\s*\([^;{}()]*\)\s*\{")


def sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(paths) > 40 and os.path.join(CSRC, LANES) in paths
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_pattern_finds_definitions_and_not_calls():
    text = sources()[LANES]
    found = set(REDUCTION.findall(text))
    assert found == {"sum_over_span", "sum_over_row16", "wave_sum", "wave_min", "wave_max", "wave_exclusive_sum", "shfl_up64", "shfl_xor64", "shfl64"}, found
    assert "sum_with_other_half" in text
    assert not REDUCTION.search("    const uint32_t n_nz = wave_sum(count);\n    if (wave_max(top) > 3u) {\n")


def test_no_other_file_defines_a_reduction():
    for name, text in sources().items():
        if name != LANES:
            assert not REDUCTION.findall(text), (name, REDUCTION.findall(text))


def test_one_frame_geometry():
    text = sources()
    assert sum(len(re.findall(r"\bstruct\s+TileFrame\s*\{", t)) for t in text.values()) == 1
    for name, t in text.items():
        assert not re.search(r"\b(?:struct|class|typedef|using)\b[^;{]*\b(?:AqFrame|LaFrame|QualityFrame)\b", t), name


def test_the_makefile_tracks_the_header():
    hdr_line = re.search(r"^HDR\s*:=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    assert "$(HERE)%s " % LANES in hdr_line
    assert '#include "%s"' % LANES in sources()["x266_device.hpp"]
