"""Every launch option on every call that reads it, loops in force: the rows, shapes and settings of tests/_option_cases.py on the
device, each result bit for bit against the CPU oracle (never against another run of the library).

include/x266hip.h promises that results never depend on the launch options.  A wrong LDS slot, unit index or loop bound under one
workgroup size or run length writes in bounds and gives a plausible frame, so per row and shape the inputs and the reference are made
once, and every setting of the row then runs the call over a seeded pre-fill with 64 bytes behind each output: the bytes the call
writes are the reference's, every other byte is still the fill, the inputs are unchanged.  Before a launch whose setting means a loop
the test asserts, with the device's own CU count, that the clamp of units_per_wave_for leaves the intended count in force -- with
"adaptive_per_wave" at its default 1 these sizes would all run one unit per wave."""
import contextlib

import numpy as np
import pytest

import _option_cases as oc
import _quant_ref as Q
import test_gpu_placement as plc
from _arena import fill_bytes
from _dev import dev, run, tile_written
from x266_amd import X266Error

gpu = pytest.mark.gpu
TAIL = 64


@contextlib.contextmanager
def _options(codec, setting):
    """the setting on top of every option's default, and whatever the context held put back afterwards"""
    saved = {k: codec.get_option(k) for k in oc.DEFAULTS}
    try:
        for k, v in dict(oc.DEFAULTS, **setting).items():
            codec.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            codec.set_option(k, v)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _code_ctu_case(oracle, size):
    """xDct32CodeCtuTilesGpu with per-region qp bytes: the reference of tests/test_gpu_quant.py"""
    w, h = size
    n = (w // 64) * (h // 64)
    cur, pred = Q._tiles_mix(w, h, 0x7000 + w + h), Q._tiles_mix(w, h, 0x7100 + w + h)
    qps = (20 + (np.arange(n * 6) * 7) % 17).astype(np.uint8)
    level, nnz, recon = Q.code_ctu_tiles(oracle, cur, pred, w, h, qps, 0, 171, base=pred)
    return plc.Case({"d_cur": cur, "d_pred": pred, "d_qp": qps},
                    {"d_level": (_bytes(level), None), "d_nnz": (_bytes(nnz.astype(np.uint32)), None), "d_recon": (_bytes(recon), tile_written(w * h // 256, "both"))},
                    lambda L, c, p: L.xDct32CodeCtuTilesGpu(c, p["d_cur"], p["d_pred"], w, h, p["d_qp"], 0, 171, p["d_level"], p["d_nnz"], p["d_recon"], None), {})


CODE_CTU_PTRS = ("d_cur", "d_pred", "d_qp", "d_level", "d_nnz", "d_recon")


def _case(oracle, row, shape):
    if row.builder == "xDct32CodeCtuTilesGpu":
        return _code_ctu_case(oracle, shape["size"]), CODE_CTU_PTRS
    r = plc.ROWS[row.builder]
    return r.build(oracle, **dict(row.fixed, **shape)), tuple(r.ptrs)


def _preconditions(codec, row, setting, shape):
    """the loop this setting is meant to run is the one in force on this device"""
    cu = codec.device_info()["cu_count"]
    assert oc.loop_length(row, setting, shape, cu) == oc.intended_length(row, setting, shape), (row.name, setting, shape, cu)


def _checked(codec, case, ptrs):
    rc = case.call(codec.L, codec.ctx, ptrs)
    if rc != 0:
        raise X266Error("%d: %s" % (rc, codec.L.xHipLastError(codec.ctx).decode()))


def _sweep_device(codec, oracle, row):
    runs = 0
    for index, shape in enumerate(row.shapes):
        case, names = _case(oracle, row, shape)
        ptrs, ins, outs = {n: None for n in names}, {}, {}
        for name, data in case.inputs.items():
            data, origin = data if isinstance(data, tuple) else (data, 0)
            ins[name] = (dev(codec, data), _bytes(data))
            ptrs[name] = ins[name][0].ptr + origin
        for k, (name, (want, written)) in enumerate(case.outputs.items()):
            fill = fill_bytes(0x0C7 + 131 * index + k, want.size + TAIL)
            outs[name] = (codec.alloc(fill.size), fill, want, slice(None) if written is None else written)
            ptrs[name] = outs[name][0].ptr
        for setting in oc.settings(row):
            _preconditions(codec, row, setting, shape)
            what = (row.name, shape, setting)
            with _options(codec, setting):
                for buf, fill, _, _ in outs.values():
                    buf.upload(fill)
                run(codec, _checked, codec, case, ptrs)
            for name, (buf, fill, want, sel) in outs.items():
                got = buf.download(np.uint8, fill.size)
                bad = np.flatnonzero(got[:want.size][sel] != want[sel])
                assert bad.size == 0, (what, name, "%d wrong byte(s), first at written byte %d, last at %d" % (bad.size, bad[0], bad[-1]))
                assert np.array_equal(got[want.size:], fill[want.size:]), (what, name, "the tail")
                if not isinstance(sel, slice):
                    assert np.array_equal(got[:want.size][~sel], fill[:want.size][~sel]), (what, name, "a hole")
            for name, (buf, data) in ins.items():
                assert np.array_equal(buf.download(np.uint8, data.size), data), (what, name, "an input")
            runs += 1
        for buf in [b[0] for b in ins.values()] + [b[0] for b in outs.values()]:
            buf.free()
    return runs


HOST = {"xDct32FwdBatch": ("dct32_fwd", 1024), "xDct32InvBatch": ("dct32_inv", 1024), "xSatd8x8Batch": ("satd8x8", 64)}   # the binding's method = the oracle's


def _sweep_host(codec, oracle, row):
    """the host-pointer calls through the binding's numpy methods: the library stages the buffers itself"""
    method, unit = HOST[row.entry]
    runs = 0
    for shape in row.shapes:
        x = plc._mixed(shape["n"], unit, 0x0C8 + shape["n"])
        keep, want = x.copy(), getattr(oracle, method)(x)
        for setting in oc.settings(row):
            _preconditions(codec, row, setting, shape)
            got = []
            with _options(codec, setting):
                run(codec, lambda: got.append(getattr(codec, method)(x)))
            assert np.array_equal(got[0].ravel(), np.asarray(want).ravel()), (row.name, shape, setting)
            assert np.array_equal(x, keep), (row.name, shape, setting)
            runs += 1
    return runs


def test_every_case_builds(oracle):
    """needs no GPU: every shape of every device row builds its inputs and its reference, on the pointers the call takes"""
    for row in oc.ROWS.values():
        if row.builder == "host":
            continue
        for shape in row.shapes:
            case, names = _case(oracle, row, shape)
            assert case.outputs and set(case.inputs) | set(case.outputs) <= set(names), (row.name, shape)
            for want, written in case.outputs.values():
                assert want.dtype == np.uint8 and want.size and (written is None or (written.size == want.size and written.any())), (row.name, shape)


@gpu
@pytest.mark.parametrize("name", list(oc.ROWS))
def test_row(codec, oracle, name):
    row = oc.ROWS[name]
    before = {k: codec.get_option(k) for k in oc.DEFAULTS}
    runs = (_sweep_host if row.builder == "host" else _sweep_device)(codec, oracle, row)
    assert runs == len(row.shapes) * len(oc.settings(row))
    assert {k: codec.get_option(k) for k in oc.DEFAULTS} == before
