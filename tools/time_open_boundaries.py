"""OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)) at 256 x 256 x 128 (Bounded, Periodic, Bounded), regular z (GPU box):
ms per RK3 step (medians of interleaved rounds of 10 steps with their range) of
  1. imposed open conditions on west and east of u, OpenBoundaryCondition(1.0): the model as it was before the scheme existed;
  2. the same model with scheme = PerturbationAdvection(0.1, Inf) on both sides: + the boundary step and the two launches of the mass-flux
     correction in each of the three pressure steps, + the carry launch where the substep rides in the tendency launch, and no replay of
     a captured step;
  3. row 1 with option use_graph = 0: what row 2 pays for not replaying a captured step, apart from its own launches;
and the time of the new launches on their own, enqueued back to back (REPS calls, one synchronise): the boundary step of the two faces
(two calls of one face each) and the flux + correction pair.
python tools/time_open_boundaries.py [rounds = 5]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=(-0.5, 0), topology=(ocn.Bounded, ocn.Periodic, ocn.Bounded))
INF = float("inf")


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]"


def make(scheme, graph=1):
    pa = ocn.PerturbationAdvection(0.1, INF) if scheme else None
    F, O_ = ocn.FieldBoundaryConditions, ocn.OpenBoundaryCondition
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"),
                                    boundary_conditions={"u": F(west=O_(1.0, scheme=pa), east=O_(1.0, scheme=pa))})
    model.set_option("use_graph", graph)
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 5)
    vals["u"] = vals["u"] + 1.0
    ocn.set_model(model, **vals)
    return model


rows = [("imposed, OpenBoundaryCondition(1.0)", make(False)), ("scheme = PerturbationAdvection(0.1, Inf)", make(True)),
        ("imposed, use_graph = 0", make(False, 0))]
dt, STEPS = 1e-4, 10
times = {name: [] for name, _ in rows}
for r in range(rounds + 1):                              # round 0 warms up (and captures the step where one is captured)
    for name, model in rows:
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            ocn.time_step(model, dt)
        ocn.synchronize()
        if r:
            times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
for name, model in rows:
    print(f"{name:45s} ms/step {med(times[name])}   scheme sides {model.get_option('open_boundary_scheme_sides')}, "
          f"graph replays {model.get_option('graph_replays')}, finite {bool(np.isfinite(model.velocities.u.interior()).all())}")
base, sch = np.median(times[rows[0][0]]), np.median(times[rows[1][0]])
print(f"scheme - imposed: {sch - base:+.3f} ms/step ({100 * (sch - base) / base:+.2f} %)")

# ---- the launches on their own
u, v, w = ocn.XFaceField(grid), ocn.YFaceField(grid), ocn.ZFaceField(grid)
u.set(1.0 + 0.01 * np.random.default_rng(1).standard_normal(grid.interior_size(u.loc)))
bc = ocn.OpenBoundaryCondition(1.0, scheme=ocn.PerturbationAdvection(0.1, INF))
REPS = 200


def timed(call):
    out = []
    for r in range(rounds + 1):
        for _ in range(5):
            call()
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        ocn.synchronize()
        if r:
            out.append((time.perf_counter() - t0) * 1e6 / REPS)
    return out


def step_both():
    ocn.kernels.step_open_boundary(u, "west", bc, 1e-4)
    ocn.kernels.step_open_boundary(u, "east", bc, 1e-4)


print(f"boundary step, west + east faces of 256 x 128 points (two launches; the model makes one): µs {med(timed(step_both))}")
print(f"flux + correction, west + east (two launches):                                        µs "
      f"{med(timed(lambda: ocn.kernels.enforce_open_boundary_mass_conservation(grid, u, v, w, {'west': bc, 'east': bc})))}")
