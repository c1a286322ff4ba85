"""The Smagorinsky eddy-viscosity kernels at 256 x 256 x 128 with tanh-stretched z (GPU box): the per-cell kernel and the marching kernel as
medians of interleaved runs with their spread, the marching kernel's rate on its algorithmic bytes, and ms per RK3 step of the configs[4]
physics with SmagorinskyLilly and with AnisotropicMinimumDissipation in the same session.
python tools/time_smagorinsky.py [rounds = 7]"""
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
F = ocn.FieldBoundaryConditions
buoyancy = ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=2e-4, haline_contraction=8e-4))
physics = dict(buoyancy=buoyancy,
               boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-4)),
                                    "T": F(top=ocn.FluxBoundaryCondition(5e-5), bottom=ocn.GradientBoundaryCondition(0.01)),
                                    "S": F(top=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(b=-1e-3 / 3600.0), field_dependencies="S"))})


def model_with(closure):
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=closure, **physics)
    ocn.set_model(m, **smooth_state({n: grid.nodes(f.loc) for n, f in m.fields().items()}, 1234))
    return m


# ---- the two kernels, interleaved
model = model_with(ocn.SmagorinskyLilly())
ocn.update_state(model, False)                      # filled halos
flds = model.fields()
nu = ocn.CenterField(grid)
variants = {"constant": (ocn.Smagorinsky(), None), "lilly_seawater": (ocn.SmagorinskyLilly(), buoyancy)}
times = {(v, k): [] for v in variants for k in (0, 1)}


def launch(v, reps):
    closure, b = variants[v]
    for _ in range(reps):
        ocn.kernels.compute_smagorinsky_viscosity(grid, closure, b, flds, flds["u"], flds["v"], flds["w"], nu)


for r in range(rounds + 1):                          # round 0 warms up
    for v in variants:
        for march in (0, 1):
            ocn.set_option("smag_march", march)
            launch(v, 3)
            ocn.synchronize()
            t0 = time.perf_counter()
            launch(v, 20)
            ocn.synchronize()
            if r:
                times[(v, march)].append((time.perf_counter() - t0) / 20 * 1e3)
ocn.set_option("smag_march", 1)
cells = N[0] * N[1] * N[2]
for v in variants:
    for march in (0, 1):
        t = np.array(times[(v, march)])
        arrays = 3 + 1 + (2 if v == "lilly_seawater" else 0)          # 3 velocity reads, the tracer reads, 1 write, 8 B per cell each
        print("%-15s %-9s median %.4f ms (min %.4f, max %.4f over %d rounds)  %.2f TB/s on %d arrays of 8 B per cell" %
              (v, "marching" if march else "per-cell", np.median(t), t.min(), t.max(), rounds, arrays * 8 * cells / (np.median(t) * 1e-3) / 1e12, arrays), flush=True)

# ---- ms per step of the configs[4] physics, SmagorinskyLilly against AMD, interleaved
del model
models = {"SmagorinskyLilly": model_with(ocn.SmagorinskyLilly()), "AnisotropicMinimumDissipation": model_with(ocn.AnisotropicMinimumDissipation())}
dt = 0.05 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
step = {n: [] for n in models}
for r in range(4):
    for n, m in models.items():
        for _ in range(3):
            ocn.time_step(m, dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, dt)
        ocn.synchronize()
        if r:
            step[n].append((time.perf_counter() - t0) / 10 * 1e3)
for n, t in step.items():
    print("%-30s %.3f ms per step (median of %s)" % (n, np.median(t), ", ".join("%.3f" % x for x in t)), flush=True)
