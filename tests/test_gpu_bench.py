"""GPU test of bench.py's plain run (no --full): the headline workload only -- the contract fields of the line, the number of timed steps as
given, none of what --full adds -- and --dump-outputs: x, y, s of the headline workload after the timed steps, float64, in the problem's sizes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cosmo_jl_amd as cj

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--small",
                        "--dump-outputs", str(tmp_path / "out")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "ADMM iterations/sec (fp64) at fixed (n,m,nnz,cone)" and out["unit"] == "ADMM iterations/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["n_gpus"] == 1 and out["steps"] == 7 and out["warmup"] == 2
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 - 1.0) < 1e-3
    assert out["config"]["workload"].startswith("cfg5") and out["roofline"] is None
    assert not {"cpu_baseline", "variants", "extra"} & set(out) and set(out["summary"]) == {"cfg5"}
    prob = cj.problems.chordal_sdp(ncliques=40, n_total=6000, n_zero=100, n_nonneg=500)          # bench.py's --small cfg5 instance
    m, n = prob["A"].shape
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("x", "y", "s")}
    assert sorted(os.listdir(tmp_path / "out")) == ["s.npy", "x.npy", "y.npy"]
    assert got["x"].shape == (n,) and got["y"].shape == (m,) and got["s"].shape == (m,)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) and np.any(a != 0) for a in got.values())
