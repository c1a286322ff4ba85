"""GPU: a plain `bench.py` run at a small size -- one JSON line with the headline keys and none of what `--full` adds -- and
`--dump-outputs`: the files hold the state the last timed step left, the same state a caller stepping the same model gets, and the
same from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("u", "v", "w", "T", "S", "pNHS")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(ocn, tmp_path):
    N, K, W = 32, 3, 1
    dumps = []
    for r in range(2):
        d = tmp_path / f"run{r}"
        out = _bench(["--gpus", "1", "--size", str(N), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(d)])
        assert out["metric"] == "cell_updates_per_s" and out["unit"] == "cell-updates/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f64" and out["steps"] == K and out["value"] > 0 and out["ms_per_step"] > 0
        assert "cpu_baseline" not in out and "ms_per_step_median" not in out and "max_abs_divergence_after_run" not in out["config"]
        dumps.append({n: np.load(d / f"{n}.npy") for n in NAMES})
    for n in NAMES:
        assert dumps[0][n].dtype == np.float64 and dumps[0][n].shape == (N, N, N), n
        assert np.array_equal(dumps[0][n], dumps[1][n]), n

    # the same model stepped here the way bench.py steps it: 2 initialisation + W warm-up steps, K steps with the tendency launches timed
    sys.path.insert(0, ROOT)
    import bench
    grid = ocn.RectilinearGrid(ocn.GPU(0), size=(N, N, N), extent=(1, 1, 1))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    ocn.set_model(model, **bench.initial_state(ocn, model))
    model.set_option("tendency_impl", 2)
    dt = 0.1 * (1.0 / N) / 0.6
    for _ in range(2 + W):
        ocn.time_step(model, dt)
    model.set_option("profile", 1)
    for _ in range(K):
        ocn.time_step(model, dt)
    model.set_option("profile", 0)
    here = bench.model_outputs(model)
    for n in NAMES:
        assert np.array_equal(here[n], dumps[0][n]), n
