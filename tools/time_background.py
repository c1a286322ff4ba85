"""background_fields at 256 x 256 x 128 with tanh-stretched z (GPU box), the `ppb_physics` coefficients of bench.py: ms per RK3 step of the
same model without backgrounds, with a background b, and with backgrounds u and b (medians of interleaved rounds of 10 steps with their
range); the same three with option fuse_substep = 0, which separates what the lost fused substep costs from what the extra advection term
costs; the time of each new launch (total velocities, term 2 for one tracer by the split role kernel and by the per-field kernel, the
four single-role split launches through the raw entry point beside today's one launch of the same four fields -- the model itself
runs a split term 1 as ONE launch over all roles, whose cost is the step-time difference between the "u and T" and the "T" models).
python tools/time_background.py [rounds = 5]"""
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
G = {n: make[n](grid) for n in "uvwc"}
bg = {n: make[n](grid) for n in "uc"}
for a in list(f.values()) + list(bg.values()):
    a.set_parent(rng.standard_normal(a.shape))
tot = ocn.XFaceField(grid)
K = ocn.kernels


def term2_tracer():
    K.compute_advective_tendency(grid, f["u"], f["v"], f["w"], bg["c"], "c", G["c"], accumulate=True)


def term1_split():
    for n in "uvwc":
        K.compute_advective_tendency(grid, f["u"], f["v"], f["w"], f[n], n, G[n])


launches = {
    "total velocity (one component)": (2, lambda: K.sum_parent(grid, f["u"], bg["u"], tot)),
    "term 2, one tracer, split role kernel": (2, term2_tracer),
    "term 2, one tracer, per-field kernel": (0, term2_tracer),
    "term 2, u, split role kernel": (2, lambda: K.compute_advective_tendency(grid, f["u"], f["v"], f["w"], bg["u"], "u", G["u"], accumulate=True)),
    "u, v, w, c: FOUR single-role split launches (raw entry)": (2, term1_split),
    "term 1 of u, v, w, c, today's role launch": (2, lambda: K.compute_tendencies(grid, f["u"], f["v"], f["w"], [f["c"]], G["u"], G["v"], G["w"], [G["c"]])),
}
times = {k: [] for k in launches}
REPS = 10
for r in range(rounds + 1):                          # round 0 warms up
    for k, (impl, fn) in launches.items():
        ocn.set_option("tendency_impl", impl)
        for _ in range(2):
            fn()
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        ocn.synchronize()
        if r:
            times[k].append((time.perf_counter() - t0) / REPS * 1e3)
ocn.set_option("tendency_impl", 2)
for k, t in times.items():
    print(f"launch  {k:50s}: {med(t)} ms")

# ---- ms per step
F = ocn.FieldBoundaryConditions
physics = dict(buoyancy=ocn.SeawaterBuoyancy(), closure=ocn.ScalarDiffusivity(ν=1e-4, κ=1e-4),
               boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-4)),
                                    "T": F(top=ocn.FluxBoundaryCondition(1e-4), bottom=ocn.GradientBoundaryCondition(0.01))})
B_bg = lambda x, y, z: 1e-2 * z + 0 * x + 0 * y          # noqa: E731
U_bg = lambda x, y, z: 0.1 * np.tanh(8 * (z + 0.5)) + 0 * x + 0 * y          # noqa: E731
variants = {"no backgrounds": None, "T": {"T": B_bg}, "u and T": {"u": U_bg, "T": B_bg}}
models, steps = {}, {}
for fuse in (1, 0):
    for name, bgs in variants.items():
        m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), background_fields=bgs, **physics)
        m.set_option("fuse_substep", fuse)
        ocn.set_model(m, **smooth_state({n: grid.nodes(fl.loc) for n, fl in m.fields().items()}, 1234))
        models[(name, fuse)], steps[(name, fuse)] = m, []
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
for (name, fuse), t in steps.items():
    m = models[(name, fuse)]
    print(f"ms/step {name:16s} fuse_substep {fuse} (active {m.get_option('fuse_substep_active')}, background path "
          f"{m.get_option('background_tendency_path')}): {med(t)}")
