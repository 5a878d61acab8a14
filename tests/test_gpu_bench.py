"""bench.py's command line on the GPU, at the small config c2 (N = 8192, M = 256, K = 4):
a plain run times its steps and nothing else, `--full` adds the side measurements, and
`--dump-outputs` writes the last timed step's results, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ("train", "k5_modes", "cpu_baseline", "kuf_hbm")
N, K = 8192, 4


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "MGP_BENCH_SHARE_GPU")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "c2", "--steps", "7", "--warmup",
                        "2", *extra], cwd=ROOT, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump(device, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = run_bench("--dump-outputs", a)
    assert line["steps"] == 7 and sum(line["steps_per_repeat"]) == 7 and line["warmup"] == 2
    assert line["unit"] == "ELBO steps/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["value"] > 0 and line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-9)
    assert line["full"] is False and line["kernels"] == {} and all(line[k] is None for k in SIDE)
    assert sorted(os.listdir(a)) == ["elbo.npy", "mu_a.npy", "mu_f.npy", "var_a.npy", "var_f.npy"]
    out = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert out["elbo"].size == 1 and float(out["elbo"].reshape(())) == line["elbo"]
    assert all(out[k].shape == (K, N) for k in ("mu_f", "var_f", "mu_a", "var_a"))
    # same arguments: same inputs, same Philox keys, same results
    assert run_bench("--dump-outputs", b)["elbo"] == line["elbo"]
    for k, v in out.items():
        np.testing.assert_array_equal(np.load(os.path.join(b, k + ".npy")), v)


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(device):
    line = run_bench("--full")
    assert line["full"] is True and line["steps"] == 7
    assert all(line[k] is not None for k in SIDE)
    assert {"expert_cond", "trsm_stats", "kuu_chol", "rbf_kuf"} <= set(line["kernels"])
    assert line["roofline"]["achieved"] > 0
