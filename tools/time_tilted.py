"""Tilted domains at 256 x 256 x 128 with tanh-stretched z (GPU box), the `ppb_physics` grid of bench.py: ms per RK3 step (medians of
interleaved rounds of 10 steps with their range) of
  1. FPlane + BuoyancyTracer + ScalarDiffusivity with option epilogue_march = 0: the per-value tendency epilogue;
  2. the same with ConstantCartesianCoriolis and a tilted gravity_unit_vector: the cost of the new terms in the same kernel form;
  3. configuration 1 with the marching epilogue (the default): what routing tilted models to the per-value form gives up;
and the time of each new stand-alone launch beside the one it joins.
python tools/time_tilted.py [rounds = 5]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state, tanh_faces
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]"


# ---- the launches, interleaved: REPS launches per timing
rng = np.random.default_rng(1)
make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}
f = {n: make[n](grid) for n in "uvwc"}
G = {n: make[n](grid) for n in "uvw"}
pHY = ocn.CenterField(grid)
for a in f.values():
    a.set_parent(rng.standard_normal(a.shape))
K = ocn.kernels
cartesian = ocn.ConstantCartesianCoriolis(fx=0.3, fy=-1.1, fz=0.7)
tilted = ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0.48, -0.6, -0.64))
launches = {
    "Coriolis, FPlane (u, v)": lambda: K.add_fplane_coriolis(grid, 0.7, f["u"], f["v"], G["u"], G["v"]),
    "Coriolis, ConstantCartesianCoriolis (u, v, w)": lambda: K.add_cartesian_coriolis(grid, cartesian, f["u"], f["v"], f["w"], G["u"], G["v"], G["w"]),
    "buoyancy acceleration (u, v)": lambda: K.add_buoyancy_acceleration(grid, tilted, {"b": f["c"]}, G["u"], G["v"]),
    "hydrostatic pressure": lambda: K.update_hydrostatic_pressure(grid, tilted.formulation, {"b": f["c"]}, pHY),
    "hydrostatic pressure, tilted": lambda: K.update_hydrostatic_pressure_tilted(grid, tilted, {"b": f["c"]}, pHY),
}
times = {k: [] for k in launches}
REPS = 10
for r in range(rounds + 1):                          # round 0 warms up
    for k, fn in launches.items():
        for _ in range(2):
            fn()
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        ocn.synchronize()
        if r:
            times[k].append((time.perf_counter() - t0) / REPS * 1e3)
for k, t in times.items():
    print(f"launch  {k:50s}: {med(t)} ms")

# ---- ms per step
closure = ocn.ScalarDiffusivity(ν=1e-4, κ=1e-4)
variants = {
    "1 FPlane, -z gravity, per-value epilogue": (ocn.FPlane(f=0.7), ocn.BuoyancyTracer(), 0),
    "2 Cartesian f, tilted gravity (per-value)": (cartesian, tilted, 0),
    "3 FPlane, -z gravity, marching epilogue": (ocn.FPlane(f=0.7), ocn.BuoyancyTracer(), 1),
}
models, steps = {}, {}
for name, (coriolis, buoyancy, march) in variants.items():
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), coriolis=coriolis, buoyancy=buoyancy, closure=closure)
    m.set_option("epilogue_march", march)
    vals = smooth_state({("T" if n == "b" else n): grid.nodes(fl.loc) for n, fl in m.fields().items()}, 1234)
    vals["b"] = 1e-2 * vals.pop("T")
    ocn.set_model(m, **vals)
    models[name], steps[name] = m, []
step_dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6
for r in range(rounds + 1):
    for key, m in models.items():
        for _ in range(2):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        if r:
            steps[key].append((time.perf_counter() - t0) / 10 * 1e3)
for name, t in steps.items():
    m = models[name]
    print(f"ms/step {name:44s} (coriolis_kind {m.get_option('coriolis_kind')}, tilted_gravity {m.get_option('tilted_gravity')}, "
          f"epilogue_march_active {m.get_option('epilogue_march_active')}): {med(t)}")
