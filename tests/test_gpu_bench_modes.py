"""bench.py's two modes: a plain run prints the headline line and nothing that takes runs of its
own; --full adds the per-kernel breakdown, the CPU baselines (and, not exercised here, the
1000-haystack leg and the side measurements)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = ["--steps", "2", "--warmup", "1", "--ramp-steps", "0", "--haystacks-per-step", "1"]
FULL_ONLY = ("batch_1000", "side_measurements", "cpu_baseline", "cpu_baseline_pow2", "cpu_baseline_config1")


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(gpu):
    d = run_bench()
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in d, key
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    for key in FULL_ONLY:
        assert key not in d, key
    assert "kernel_ms_per_haystack" not in d["roofline_pipeline"] and "dominant_by_time" not in d["roofline_pipeline"]


def test_full_run_adds_the_breakdown_and_the_cpu_baselines(gpu):
    d = run_bench("--full", "--no-batch-1000", "--no-extra-legs", "--cpu-chunks", "1")
    kern = d["roofline_pipeline"]["kernel_ms_per_haystack"]
    assert set(kern) == {"k1_cols_fwd", "k2_rows", "k3_cols_inv", "tile_stats", "peaks"}
    assert kern["k2_rows"] > 0 and d["roofline_pipeline"]["dominant_by_time"] in kern
    for key in ("cpu_baseline", "cpu_baseline_pow2", "cpu_baseline_config1"):
        assert d[key]["value"] > 0 and "offsets_ok=True" in d[key]["sample"], (key, d[key])
    assert "batch_1000" not in d and "side_measurements" not in d
