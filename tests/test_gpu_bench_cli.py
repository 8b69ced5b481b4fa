"""bench.py's command line: a plain run prints the headline fields only and
``--dump-outputs`` writes the last timed step's results; ``--full`` adds the
profiled pass.  Each run is a fresh ``python bench.py`` process (the command
line is what is under test), a few steps each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "kernels_ms_per_step", "cpu_baseline", "extra_workloads")
DUMPED = {"cx": (11,), "cy": (11,), "cost_lane": (), "cost_obs": (), "sigma": (), "res_beta": (20,), "beta": (22,)}


def _line(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(bench.ROOT, "bench.py"), "--gpus", "1", *argv], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1
    return json.loads(out[0])


def test_plain_run_and_dump(tmp_path):
    dumps = []
    for d in ("a", "b"):
        line = _line("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
        assert line["steps"] == 3 and line["unit"] == "steps/s" and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["metric"] == bench.METRIC
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
        assert not [k for k in FULL_ONLY if k in line]
        assert sorted(os.listdir(tmp_path / d)) == sorted(f"{k}.npy" for k in DUMPED)
        dumps.append({k: np.load(tmp_path / d / f"{k}.npy") for k in DUMPED})
    for k, shape in DUMPED.items():
        a, b = dumps[0][k], dumps[1][k]
        assert a.dtype == np.float32 and a.shape == shape and np.all(np.isfinite(a))
        assert np.array_equal(a, b), k   # same arguments: same inputs, same outputs


def test_full_adds_the_profiled_pass():
    line = _line("--steps", "2", "--warmup", "1", "--full", "--profile-steps", "1", "--cpu-seconds", "0",
                 "--extra", "0")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] in line["kernels_ms_per_step"]
    assert all(v > 0 for v in line["kernels_ms_per_step"].values())
