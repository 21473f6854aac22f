"""CPU: the argument rules of the calls that take their device pointers in a host-read struct (x266_amd/csrc/x266_args.hpp: the compact
level stream, source analysis, lookahead, the seeded search, the mixed frame, RDOQ) and of xWeightsFromTotals and xSceneCutFromTotals,
against the contract as tests/cpp/struct_rules_check.cpp writes it down: one description per struct, one walk of single perturbations of
a base tuple with and without the optional buffers, made-up addresses, extents that saturate, the largest frame an int describes.  The
driver is a stand-alone program, built twice -- plain, and with the address and undefined-behaviour sanitizers.  The table of
tests/cpp/arg_rules_check.cpp does not count these calls; tests/test_{levels,aq,la,seed,mixed,rdoq}_arg_rules.py hold each family's
surface and compare the driver's per-call lines with the header.  g++ only: no GPU, no HIP."""
import re

import _cpp_driver

# the checks the finished driver prints per family (896, 556, 12818, 1089, 2565, 1076): a walk that shrank must not pass quietly
CHECK_FLOORS = {"x266_levels_t": 890, "x266_aq_t": 550, "x266_la_t": 12800, "x266_seed_t": 1080, "x266_mixed_t": 2560, "x266_rdoq_t": 1070}
STRUCT_CALLS = ("xLevelsPackGpu", "xLevelsUnpackGpu", "xAqStatsGpu", "xAqDecideGpu", "xLaDownscaleGpu", "xLaIntraCostsGpu", "xLaFrameCostGpu", "xLaPropagateGpu",
                "xLaTreeQpGpu", "xSatd8x8SeededSearchGpu", "xDct32CodeMixedFrameGpu", "xRdoQuantRegionsGpu", "xLevelsBitsGpu")


@_cpp_driver.needs_gxx
def test_the_rules_hold():
    text = _cpp_driver.struct_rules_output()
    checks = {name: int(n) for name, n in re.findall(r"^checks (\w+) (\d+)$", text, re.M)}
    assert set(checks) == set(CHECK_FLOORS), sorted(checks)
    for family, floor in CHECK_FLOORS.items():
        assert checks[family] >= floor, (family, checks[family])
    assert set(_cpp_driver.struct_call_lines()) == set(STRUCT_CALLS)        # every struct call has its row in the driver


@_cpp_driver.needs_gxx
def test_the_rules_hold_under_the_sanitizers(tmp_path):
    _cpp_driver.build_and_run_sanitized(tmp_path, "struct_rules_check")
