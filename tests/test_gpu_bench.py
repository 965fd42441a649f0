"""bench.py on the GPU: a plain run times --steps steps and prints the
headline line only, --dump-outputs writes what the last timed step computed,
and --full adds the profiled pass's tables."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps")
FULL_ONLY = ("kernels", "roofline", "profiled_ms_per_step", "cpu_baseline", "dp")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--frames-per-gpu", "64", *extra],
                       env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(tmp_path):
    import bench
    out = tmp_path / "dump"
    res = _bench("--dump-outputs", str(out))
    for k in HEADLINE:
        assert k in res, k
    for k in FULL_ONLY:
        assert k not in res, k
    assert res["steps"] == 3 and res["unit"] == "frames/sec" and res["dtype"] == "f32"
    assert res["value"] > 0 and res["higher_is_better"] is True
    # value and ms_per_step describe the same 3 timed steps of 64 frames
    assert res["value"] == pytest.approx(64 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    share = bench.DUMP_BUDGET_BYTES // 4 // 6
    n_fc = bench.POOL_OUT * bench.FC_OUT
    assert n_fc > share
    shapes = {"output": (64, bench.FC_OUT), "input_deriv": (64, bench.H * bench.W * bench.C),
              "component0_linear_params": (bench.G, bench.KH * bench.KW * bench.C),
              "component0_bias_params": (bench.G,),
              "component2_linear_params": (share,), "component2_bias_params": (bench.FC_OUT,)}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float32 and sorted(a.shape) == sorted(shape), (name, a.shape)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    assert res["dumped_outputs"]["component2_linear_params"] == [share, n_fc]


def test_full_run_adds_the_profiled_tables():
    res = _bench("--full", "--no-cpu-baseline")
    for k in HEADLINE + ("kernels", "roofline", "profiled_ms_per_step"):
        assert k in res, k
    assert res["kernels"] and res["roofline"]["kernel"] in res["kernels"]
