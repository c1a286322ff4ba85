"""The dynamic Smagorinsky coefficient at 256 x 256 x 128 on the (Periodic, Periodic, Bounded) grid with tanh-stretched z (GPU box): ms per
coefficient update for averaging = (1, 2) and for LagrangianAveraging (the averaging branch), and ms per RK3 step with IterationInterval(1)
and IterationInterval(5), against the constant-coefficient Smagorinsky model in the same session; interleaved runs, medians with the spread.
python tools/time_dynamic_smagorinsky.py [rounds = 7]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state, tanh_faces
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))


def model_with(closure):
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=closure)
    ocn.set_model(m, **smooth_state({n: grid.nodes(f.loc) for n, f in m.fields().items()}, 1234))
    return m


# ---- one coefficient update, the two averagings interleaved
model = model_with(ocn.Smagorinsky())
ocn.update_state(model, False)                      # filled halos
u, v, w = model.velocities
coefficients = {"averaging=(1, 2)": ocn.DynamicCoefficient(averaging=(1, 2)), "LagrangianAveraging": ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging())}
fields = {n: ocn.kernels.dynamic_coefficient_fields(grid, c) for n, c in coefficients.items()}
dt = 0.05 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
for n, c in coefficients.items():                    # the Lagrangian fields start from their initialising update
    ocn.kernels.dynamic_smagorinsky_update(grid, c, u, v, w, fields[n])
times = {n: [] for n in coefficients}
for r in range(rounds + 1):                          # round 0 warms up
    for n, c in coefficients.items():
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            ocn.kernels.dynamic_smagorinsky_update(grid, c, u, v, w, fields[n], Δt=dt, initialising=False)
        ocn.synchronize()
        if r:
            times[n].append((time.perf_counter() - t0) / 5 * 1e3)
for n, t in times.items():
    t = np.array(t)
    print("coefficient update  %-20s median %.3f ms (min %.3f, max %.3f over %d rounds; with the call's scratch allocation)" %
          (n, np.median(t), t.min(), t.max(), rounds), flush=True)

# ---- ms per RK3 step, interleaved
del model, fields
I = ocn.IterationInterval
closures = {"Smagorinsky (constant)": ocn.Smagorinsky(),
            "dynamic (1, 2), every step": ocn.DynamicSmagorinsky(averaging=(1, 2)),
            "dynamic (1, 2), every 5th": ocn.DynamicSmagorinsky(averaging=(1, 2), schedule=I(5)),
            "dynamic Lagrangian, every step": ocn.DynamicSmagorinsky(averaging=ocn.LagrangianAveraging()),
            "dynamic Lagrangian, every 5th": ocn.DynamicSmagorinsky(averaging=ocn.LagrangianAveraging(), schedule=I(5))}
models = {n: model_with(c) for n, c in closures.items()}
step = {n: [] for n in models}
for r in range(rounds + 1):                          # round 0 warms up
    for n, m in models.items():
        for _ in range(5 if r == 0 else 0):
            ocn.time_step(m, dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, dt)
        ocn.synchronize()
        if r:
            step[n].append((time.perf_counter() - t0) / 10 * 1e3)
for n, t in step.items():
    t = np.array(t)
    print("%-32s median %.3f ms per step (min %.3f, max %.3f over %d rounds)" % (n, np.median(t), t.min(), t.max(), rounds), flush=True)
