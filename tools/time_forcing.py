"""ms per RK3 time-step at 256^3 (configs[1]: triply periodic, WENO5, two tracers) with and without forcing (GPU box):
unforced; a z-GaussianMask sponge with a LinearTarget on all five fields; Forcing(array) on T and S. Interleaved repetitions, median."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oldoceananigans_jl_amd as ocn   # noqa: E402
from helpers import smooth_state     # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS, REPS = (20, 3) if N >= 256 else (100, 3)
arch = ocn.GPU(0)
grid = ocn.RectilinearGrid(arch, size=(N, N, N), extent=(1, 1, 1))
sponge = ocn.Relaxation(rate=1 / 60, mask=ocn.GaussianMask("z", center=-1.0, width=0.1),
                        target=ocn.LinearTarget("z", intercept=0.0, gradient=1e-3))
arr = np.random.default_rng(0).standard_normal((N, N, N)) * 1e-3
cases = {"unforced": None, "sponge (5 fields)": {n: sponge for n in ("u", "v", "w", "T", "S")}, "array (T, S)": {"T": arr, "S": arr}}
models = {}
for name, forcing in cases.items():
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), forcing=forcing)
    ocn.set_model(m, **smooth_state({n: grid.nodes(f.loc) for n, f in m.fields().items()}, 1234))
    models[name] = m
dt = 0.1 / N / 0.6
times = {name: [] for name in cases}
for _ in range(REPS):
    for name, m in models.items():
        for _ in range(3):
            ocn.time_step(m, dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            ocn.time_step(m, dt)
        ocn.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / STEPS)
base = float(np.median(times["unforced"]))
for name, t in times.items():
    med = float(np.median(t))
    print(f"{N}^3 {name:18s} {med:7.3f} ms/step  ({100 * (med / base - 1):+5.1f} %)  forcing_path {models[name].get_option('forcing_path')}",
          flush=True)
