"""GPU: bench.py end to end at a small size -- every leg runs, the JSON line carries the contract's fields,
and the CPU-baseline leg confirms the GPU output bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _util import ROOT

pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _line_and_full(out, cwd):
    """stdout = exactly one compact JSON line (what the driver parses: < 8 KB, the contract's keys); the full record is the file it names"""
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.count("\n") == 1 and out.stdout.startswith("{"), out.stdout[-2000:]
    assert len(out.stdout) < 8192, len(out.stdout)
    line = json.loads(out.stdout)
    for k in CONTRACT:
        assert k in line, k
    full = json.load(open(os.path.join(cwd, line["full_record"])))
    for k in ("metric", "value", "n_gpus", "steps", "warmup", "ms_per_step", "output_checksum_sum_i16"):
        assert line[k] == full[k], k
    assert abs(line["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-4
    return line, full


def _run(args, tmp):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=tmp, capture_output=True, text=True, timeout=900)
    return _line_and_full(out, tmp)


def test_bench_small_run_has_every_leg_and_field(tmp_path):
    line, d = _run(["--full", "--steps", "3", "--warmup", "1", "--dct-blocks", "8192", "--satd-blocks", "131072"], str(tmp_path))
    for k in CONTRACT:
        assert k in d, k
    # the driver's line: numbers only, every leg as one scalar, every boolean check of the run green, the chip named
    assert line["checks_failed"] == [] and "error" not in line and "MI355" in line["device"]
    assert line["roofline"]["traffic"] == pytest.approx(d["roofline"]["traffic"], rel=1e-4) if d["roofline"]["traffic"] else line["roofline"]["traffic"] is None
    assert line["cpu_baseline"]["kind"] in ("reference", "port") and line["cpu_baseline"]["gpu_output_bit_exact_vs_cpu"] is True
    for leg in ("dct32_inv", "dct32_fwd_inv_fused", "satd8x8", "satd8x8_me_search", "stream8k", "per_ctu_one_launch"):
        assert isinstance(line["also"][leg], float), leg
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and d["scaling"] == "weak" and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["cpu_baseline"]["gpu_output_bit_exact_vs_cpu"] is True and d["cpu_baseline"]["cores"] >= 1
    for leg in ("dct32_inv", "dct32_fwd_inv_fused", "satd8x8", "satd8x8_me_search", "sad8x8_me_search", "transform_set",
                "fused_from_tiles", "front_end_and_sad", "intra32", "stream8k", "dct32_scatter_gather", "satd8x8_me_search_sharded"):
        assert leg in d["also"], leg
    # kernel time and wall-clock come from the same launches: the former can never exceed the latter
    assert r["kernel_ms_per_launch"] <= d["ms_per_step"] * 1.0001
    for leg in ("dct32_inv", "dct32_fwd_inv_fused", "satd8x8", "satd8x8_me_search"):
        assert d["also"][leg]["kernel_ms_mean"] <= d["also"][leg]["ms_per_step"] * 1.0001, leg
    # the same-run ceilings of THIS box and every HBM-bound leg expressed in them (round 4)
    sb = r["same_box"]
    for k in ("copy_TBps", "read_TBps", "read_no_store_TBps", "write_TBps"):      # 16 MiB buffers here: launch-bound, only sanity (the full-size
        assert 0.5 < sb[k] < 8.0, (k, sb)                                           # streams are asserted in tests/test_gpu_perf_floor.py)
    # (presence and sign only: at this size the streams run on 16 MiB and the SATD batch on 8 MiB, cache-resident and launch-bound,
    #  so the ratios mean nothing -- 0.4 .. 1.7 seen; tests/test_gpu_perf_floor.py asserts them at full size)
    assert r["frac_of_same_box_copy"] > 0 and d["also"]["satd8x8"]["roofline"]["frac_of_same_box_read"] > 0
    assert "frac_of_same_box_copy" in d["also"]["dct32_fwd_inv_fused"] and "frac_of_same_box_write" in d["also"]["intra32"]["predict"]
    # the literal drop-in path (host pointers): PCIe-inclusive, next to what the link gives
    h = d["also"]["host_api"]
    assert h["pinned"]["same_result_as_pageable"] is True and h["pinned"]["GBps_each_way"] > 5 and h["link_GBps"]["each_way_both_directions_at_once"] > 5
    # HBM bytes per launch: measured in this run by two rocprofv3 --pmc passes (counter factors calibrated on a copy of known size), or an honest label why not
    assert r["traffic_source"]
    if r["traffic"] is not None and "measured in this run" in r["traffic_source"]:
        assert 0.98 <= r["traffic"] / r["algorithmic_bytes_per_launch"] <= 1.10, r
    assert d["also"]["stream8k"]["bit_exact_vs_single_device"] is True          # BASELINE configs[4] through the C node layer
    assert d["also"]["satd8x8_me_search_sharded"]["identical_to_single_device"] is True
    assert 0 < d["cpu_baseline"]["parallel_efficiency"] < 4 and d["cpu_baseline"]["host_cpu"]
    assert d["also"]["dct32_fwd_inv_fused"]["same_bytes_as_two_kernels"] is True
    assert d["also"]["satd8x8_me_search"]["planted_mv_found_fraction"] > 0.99
    assert "error" not in d


def test_bench_plain_run_is_the_headline_only_and_dumps_its_outputs(tmp_path):
    """without --full: the headline's K timed steps and nothing else; --dump-outputs writes the seeded sample of the last step's
    coefficients, which are the oracle's transform of the same seeded inputs"""
    import bench
    from _util import Oracle, residual_np
    n, tmp = 20000, str(tmp_path)
    line, d = _run(["--steps", "7", "--warmup", "2", "--dct-blocks", str(n), "--dump-outputs", os.path.join(tmp, "out")], tmp)
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "blocks/s"
    assert d["metric"] == "dct32_fwd_blocks_per_s" and d["higher_is_better"] is True and d["dtype"] == "i32"
    assert "also" not in d and d["cpu_baseline"] is None and d["roofline"]["same_box"] is None and d["roofline"]["traffic"] is None
    assert line["roofline"]["kernel_ms_per_launch"] <= line["ms_per_step"] * 1.0001
    assert os.listdir(os.path.join(tmp, "out")) == ["dct32_fwd_coefficients.npy"]
    got = np.load(os.path.join(tmp, "out", "dct32_fwd_coefficients.npy"))
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_BLOCKS, 1024)
    blocks = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, bench.DUMP_BLOCKS, replace=False))
    x = residual_np(n * 1024, bench.DCT_SEED).reshape(n, 1024)[blocks]
    assert np.array_equal(got, Oracle().dct32_fwd(x).astype(np.float32))


def test_bench_two_ranks_share_the_gpu_and_agree_with_one_rank(tmp_path):
    """The N > 1 path of bench.py on a one-GPU box (X266_BENCH_SHARE_GPU: ranks share the device, control plane on gloo):
    every rank transforms its own slice of the one seeded stream, so two ranks x n blocks must give the output checksum
    of one rank x 2n blocks; the JSON reports n_gpus = 2 and the whole-job rate."""
    n = 16384
    tmp = str(tmp_path)
    _, one = _run(["--full", "--steps", "3", "--warmup", "1", "--dct-blocks", str(2 * n), "--no-also", "--no-cpu-baseline", "--no-live-traffic"], tmp)
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, X266_BENCH_SHARE_GPU="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "3", "--warmup", "1",
                          "--dct-blocks", str(n), "--no-also", "--no-cpu-baseline"], cwd=tmp, env=env, capture_output=True, text=True, timeout=900)
    line2, two = _line_and_full(out, tmp)                           # rank 0 only
    assert len(line2["roofline"]["frac_by_rank"]) == 2 and line2["cpu_baseline"] is None
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["cpu_baseline"] is None
    assert two["output_checksum_sum_i16"] == one["output_checksum_sum_i16"]
    assert two["config"]["blocks_per_gpu"] == n
    assert len(two["roofline"]["frac_by_rank"]) == 2 and min(two["roofline"]["frac_by_rank"]) > 0
    # the same job WITHOUT torchrun on the command line: plain `python bench.py --gpus 2` spawns its own ranks (how a scaling harness
    # that re-uses the single-GPU command shape would call it)
    env2 = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "3", "--warmup", "1",
                          "--dct-blocks", str(n), "--no-also", "--no-cpu-baseline"], cwd=tmp, env=env2, capture_output=True, text=True, timeout=900)
    _, self_spawned = _line_and_full(out, tmp)
    assert self_spawned["n_gpus"] == 2 and self_spawned["output_checksum_sum_i16"] == one["output_checksum_sum_i16"]


@pytest.mark.parametrize("ranks", [2, 4, 8])
def test_bench_node_legs_with_one_process_per_rank_under_the_rccl_model(ranks, tmp_path):
    """bench.py --gpus N with its node-layer legs (stream8k, scatter-gather, sharded search) in N processes on this one GPU:
    control plane on gloo, the library's RCCL calls served by tests/rccl_model (multi-process mode).  The rates mean
    nothing here; the legs must complete, match the single-device results, and leave exactly one compact JSON line --
    the command shape the driver's 1/2/4/8 scaling run uses (no 8-GPU node has been available to any round)."""
    model = os.path.join(ROOT, "tests", "rccl_model", "librccl_model.so")
    assert os.path.exists(model)
    tmp = str(tmp_path)
    env = dict(os.environ, X266_BENCH_SHARE_GPU="1", X266HIP_RCCL_LIB=model, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    # no torchrun on the command line: bench.py --gpus N spawns its own ranks
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--full", "--steps", "3", "--warmup", "1",
                          "--dct-blocks", "16384", "--satd-blocks", "65536", "--stream8k", "6", "--no-transform-set", "--no-cpu-baseline"],
                         cwd=tmp, env=env, capture_output=True, text=True, timeout=1500)
    line, d = _line_and_full(out, tmp)
    also = d["also"]
    assert "node_layer_error" not in also and "node_layer_error" not in line, also.get("node_layer_error")
    assert line["n_gpus"] == ranks and line["rccl_ranks"] == ranks and line["checks_failed"] == [] and line["cpu_baseline"] is None
    assert len(line["roofline"]["frac_by_rank"]) == ranks
    assert also["stream8k"]["bit_exact_vs_single_device"] is True and also["stream8k"]["frames"] == 6
    assert also["dct32_scatter_gather"]["value"] > 0
    # the N > 1 record carries what a reader needs to judge the multi-device numbers: per-rank roofline fractions, the RCCL every rank
    # talks to, and the measured end-to-end rates NEXT TO the per-link prediction (153 GB/s per direction and peer)
    assert len(d["roofline"]["frac_by_rank"]) == ranks and len(also["rccl_by_rank"]) == ranks
    assert also["dct32_scatter_gather"]["link_bound_blocks_per_s"] == pytest.approx(ranks * 153e9 / 2048)
    assert also["stream8k"]["link_bound_frames_per_s"] == pytest.approx(153e9 / ((32400 * 2048 + 518400 * 128) / ranks))
    assert also["satd8x8_me_search_sharded"]["identical_to_single_device"] is True and also["satd8x8_me_search_sharded"]["stripes"] == ranks


def test_bench_prints_its_line_when_a_peer_never_joins(tmp_path):
    """A rank that never reaches the node layer (RCCL hang, dead peer): the other rank's communicator setup blocks; past --node-timeout
    every rank's watchdog fires, rank 0 prints the compact line WITHOUT the node legs (error named) and the job ends -- no hang, exit 0."""
    import time
    model = os.path.join(ROOT, "tests", "rccl_model", "librccl_model.so")
    tmp = str(tmp_path)
    env = dict(os.environ, X266_BENCH_SHARE_GPU="1", X266HIP_RCCL_LIB=model, HSA_ENABLE_IPC_MODE_LEGACY="0", X266_BENCH_TEST_STALL_RANK="1")
    env = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "3", "--warmup", "1", "--dct-blocks", "16384",
                          "--satd-blocks", "65536", "--stream8k", "6", "--no-transform-set", "--no-me", "--no-cpu-baseline", "--node-timeout", "10"],
                         cwd=tmp, env=env, capture_output=True, text=True, timeout=300)
    took = time.time() - t0
    line, full = _line_and_full(out, tmp)
    assert took < 120, took
    assert "did not finish within 10 s" in line["node_layer_error"] and "stream8k" not in line["also"]
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["also"]["dct32_inv"] > 0       # the legs before the node layer are all there
