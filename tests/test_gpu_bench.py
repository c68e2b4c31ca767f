"""GPU: bench.py end to end at a small size.  A plain run measures and reports the headline only; --full adds the
other measurements to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IPXK_FORCE_COMM")}
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                         "--rows", "20000", "--cols", "40000"] + list(extra),
                        capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert pr.returncode == 0, pr.stderr[-3000:]
    return json.loads(pr.stdout.strip().splitlines()[-1])


def check_headline(out):
    assert out["metric"] == "kkt_solves_per_sec" and out["unit"] == "solves/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    assert out["config"]["errflag"] == 0 and out["config"]["cr_iterations_per_solve"] > 0
    assert out["summary"]["headline_solves_per_s"] == out["value"]


def test_plain_run_reports_the_headline_only(tmp_path):
    out = run_bench("--dump-outputs", str(tmp_path))
    check_headline(out)
    assert out["full"] is False and out["cpu_baseline"] is None and "roofline" not in out
    extra = {"basis_path", "lu_path", "maxvolume_path", "newton_step", "parity_vs_cpu", "other_configs", "model_upload"}
    assert not extra & set(out["config"])
    x, y = np.load(tmp_path / "x.npy"), np.load(tmp_path / "y.npy")
    assert x.size == 40000 + 20000 and y.size == 20000 and np.isfinite(x).all() and np.isfinite(y).all()
    assert list(np.load(tmp_path / "iterations_errflag.npy")) == [out["config"]["cr_iterations_per_solve"], 0]


def test_full_run_adds_the_other_measurements():
    out = run_bench("--full", "--no-other-configs")
    check_headline(out)
    assert out["full"] is True
    assert out["roofline"]["us_per_apply"] > 0 and "banded_matrix_probe" in out["roofline"]
    assert out["cpu_baseline"]["value"] > 0
    for k in ("basis_path", "lu_path", "maxvolume_path", "newton_step", "parity_vs_cpu", "model_upload"):
        assert k in out["config"], k
    assert "apply_us" in out["summary"]
