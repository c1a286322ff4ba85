"""The vertically implicit solve at 256 x 256 x 128 with tanh-stretched z (GPU box): time per launch of every form the library has (FORMS;
form 0, the reference-shaped kernel, is the one shipped) for a Center and a Face field, as medians of interleaved runs with their
range, the rate on the 16 B per cell floor, and ms per RK3 step of the ppb_physics configuration with the ScalarDiffusivity explicit and
vertically implicit in the same session.
python tools/time_vertically_implicit.py [rounds = 7]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state, tanh_faces
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
FORMS = (0,)                                          # add a candidate form here to time it against the shipped one, alternating
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
cells = N[0] * N[1] * N[2]
dzmin = float(np.min(grid.Δzᵃᵃᶜ[grid.Hz:grid.Hz + grid.Nz]))
kappa, dt = 1e-3, 50 * dzmin ** 2 / 1e-3

# ---- the forms of the solve, interleaved
fields = {"center": ocn.CenterField(grid), "face": ocn.ZFaceField(grid)}
rng = np.random.default_rng(1)
for f in fields.values():
    f.set_parent(rng.standard_normal(f.shape))
times = {(n, form): [] for n in fields for form in FORMS}
REPS = 20
for r in range(rounds + 1):                          # round 0 warms up
    for n, f in fields.items():
        for form in FORMS:
            for _ in range(3):
                ocn.kernels.implicit_step(grid, f, kappa, dt, form=form)
            ocn.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                ocn.kernels.implicit_step(grid, f, kappa, dt, form=form)
            ocn.synchronize()
            if r:
                times[(n, form)].append((time.perf_counter() - t0) / REPS * 1e3)
for (n, form), t in times.items():
    t = np.array(t)
    print(f"implicit_step {n:6s} form {form}: median {np.median(t) * 1e3:7.1f} us  range [{t.min() * 1e3:.1f}, {t.max() * 1e3:.1f}] us  "
          f"{16 * cells / (np.median(t) * 1e-3) / 1e12:.2f} TB/s on the 16 B/cell floor")

# ---- ms per step: the ppb_physics configuration (bench.py's grid and coefficients), explicit and vertically implicit
F = ocn.FieldBoundaryConditions
physics = dict(buoyancy=ocn.SeawaterBuoyancy(),
               boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-4)),
                                    "T": F(top=ocn.FluxBoundaryCondition(1e-4), bottom=ocn.GradientBoundaryCondition(0.01))})
steps = {}
models = {}
for how in ("explicit", "vertically_implicit"):
    td = ocn.VerticallyImplicitTimeDiscretization() if how == "vertically_implicit" else ocn.ExplicitTimeDiscretization()
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.ScalarDiffusivity(td, ν=1e-4, κ=1e-4), **physics)
    ocn.set_model(m, **smooth_state({n: grid.nodes(f.loc) for n, f in m.fields().items()}, 1234))
    models[how], steps[how] = m, []
step_dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6
for r in range(rounds + 1):
    for how, m in models.items():
        for _ in range(2):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        if r:
            steps[how].append((time.perf_counter() - t0) / 10 * 1e3)
for how, t in steps.items():
    t = np.array(t)
    print(f"ms/step {how:20s}: median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]  (form {models[how].get_option('implicit_step_form')})")
