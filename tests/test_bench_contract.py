"""bench.py's driver contract, checked on CPU: the default workload is BASELINE.json's
headline configuration (configs[1]) and the metric string is BASELINE.json's."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_metric_is_baselines():
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert bench.METRIC == base["metric"]


def test_default_workload_is_cfg2(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.k, a.sn, a.sl, a.lim) == (1, 16, 10_000, 100, 500)
    assert a.scaling == "weak"  # every rank its own sn reads (per-GPU work fixed)
    assert a.steps > 0 and a.warmup >= 0


def test_config_overrides(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "cfg5", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.k, a.sn, a.sl, a.lim, a.steps, a.warmup) == (22, 100_000, 150, 1000, 3, 1)
    assert a.read_len >= 2 * a.sl  # every read long enough for both ends


def test_cfg4_is_strong_scaling(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "cfg4"])
    a = bench.parse()
    assert (a.k, a.sn, a.sl, a.lim, a.scaling) == (16, 1_000_000, 100, 500, "strong")


def test_plain_run_times_the_stage_alone(monkeypatch):
    """Without --full none of the legs beside the headline figure runs; with it each one does
    unless its own --no-... option is given."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and not a.verify
    assert a.no_kernel_leg and a.no_pipelined and a.no_exact and a.no_cpu_baseline
    assert (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-exact", "--dump-outputs", "some/dir"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "some/dir"
    assert a.no_exact and not (a.no_kernel_leg or a.no_pipelined or a.no_cpu_baseline)


def test_workload_is_the_same_from_run_to_run():
    """--dump-outputs compares two builds output for output: the same arguments give the same inputs."""
    import argparse

    import numpy as np

    args = argparse.Namespace(k=16, sn=300, sl=100, lim=50, read_len=400, seed=1, scaling="weak")
    a, units_a = bench.build_workload(args, 0, 1)
    b, units_b = bench.build_workload(args, 0, 1)
    assert units_a == units_b > 0
    for e in ("start", "end"):
        assert np.array_equal(a[e]["kmers"], b[e]["kmers"])
        assert len(a[e]["windows"]) == len(b[e]["windows"])
        assert all(np.array_equal(x, y) for x, y in zip(a[e]["windows"], b[e]["windows"]))


def test_cpu_share_reports_nproc():
    n, quota = bench.cpu_share()
    assert n == len(os.sched_getaffinity(0))
    assert quota is None or quota > 0


def test_stage_text_says_what_runs():
    """config.stage describes the timed step as it runs: the count launch is issued first in each
    call (the armed launch, which enqueued it during the previous step, was removed in ABI 6)."""
    for world in (1, 2):
        t = bench.stage_text("early-launch", world)
        assert "issued first in the call" in t
        assert "armed" not in t and "previous step" not in t
    assert "DMA" in bench.stage_text("dma", 1)
    assert bench.stage_text("early-launch", 2).endswith("RCCL all-reduce -> counts D2H")
