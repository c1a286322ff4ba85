"""ImmersedBoundaryGrid at 256 x 256 x 128 with tanh-stretched z (Periodic, Periodic, Bounded), RK3, no physics beside WENO advection of two
tracers (GPU box): ms per step of
  * the plain model at halo (4, 4, 4),
  * the same grid wrapped with an empty boundary (a bottom below the domain): what the immersed composition itself costs -- the per-field
    tendency kernels with their flag loads, the two mask launches, substeps and halo fills as launches of their own,
  * a Gaussian seamount reaching a third of the depth on immersed tendency path 2 (the flux-sharing role kernel) and on path 1 (one field
    per launch, tendency_impl = 0),
and the launches, timed alone: the four per-field tendency kernels (u, v, w, one tracer) on the plain grid and their immersed instantiations on
the seamount grid, and mask_immersed_field of one field. Medians of interleaved rounds of 10 steps with their range; host clock around work that ends in a device synchronise.
python tools/time_immersed.py [rounds = 5]"""
import sys, os, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state, tanh_faces
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)


def plain_grid():
    return ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=tanh_faces(N[2]), halo=(4, 4, 4), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]"


seamount = lambda x, y: -1.0 + (1.0 / 3.0) * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / (2 * 0.1 ** 2))          # noqa: E731
grids = {"plain": plain_grid(),
         "empty boundary": ocn.ImmersedBoundaryGrid(plain_grid(), ocn.GridFittedBottom(-2.0)),
         "seamount, path 2": ocn.ImmersedBoundaryGrid(plain_grid(), ocn.GridFittedBottom(seamount)),
         "seamount, path 1": ocn.ImmersedBoundaryGrid(plain_grid(), ocn.GridFittedBottom(seamount))}
models, steps = {}, {}
for name, grid in grids.items():
    ocn.set_option("tendency_impl", 0 if name.endswith("path 1") else 2)          # (a model copies the library default when it is created)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"))
    ocn.set_option("tendency_impl", 2)
    ocn.set_model(m, **smooth_state({n: grid.nodes(fl.loc) for n, fl in m.fields().items()}, 1234))
    models[name], steps[name] = m, []
    if name != "plain":
        cells = grid.immersed_cell_mask()[4:-4, 4:-4, 4:-4]
        print(f"{name}: {int(cells.sum())} of {cells.size} cells immersed, tendency path {m.get_option('immersed_tendency_path')}")
step_dt = 0.1 * grids["plain"].Δxᶜᵃᵃ / 0.6
for r in range(rounds + 1):                          # round 0 warms up
    for name, m in models.items():
        for _ in range(2):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        if r:
            steps[name].append((time.perf_counter() - t0) / 10 * 1e3)
for name, t in steps.items():
    print(f"ms/step {name:18s}: {med(t)}")

# ---- the launches, alone
ibg = grids["seamount, path 1"]
make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}
rng = np.random.default_rng(1)
K = ocn.kernels
launches = {}
for label, grid in (("plain", grids["plain"]), ("immersed", ibg)):
    f = {n: make[n](grid) for n in "uvwc"}
    G = {n: make[n](grid) for n in "uvwc"}
    for a in f.values():
        a.set_parent(rng.standard_normal(a.shape))
    if label == "immersed":
        launches["u, v, w, c tendencies, flux-sharing role kernel, immersed"] = (
            2, lambda grid=grid, f=f, G=G: K.compute_tendencies(grid, f["u"], f["v"], f["w"], [f["c"]], G["u"], G["v"], G["w"], [G["c"]]))
    launches[f"u, v, w, c tendencies, per-field kernels, {label}"] = (
        0, lambda grid=grid, f=f, G=G: (K.compute_Gu(grid, f["u"], f["v"], f["w"], G["u"]), K.compute_Gv(grid, f["u"], f["v"], f["w"], G["v"]),
                                        K.compute_Gw(grid, f["u"], f["v"], f["w"], G["w"]), K.compute_Gc(grid, f["u"], f["v"], f["w"], f["c"], G["c"])))
    if label == "immersed":
        launches["mask_immersed_field of one field"] = (0, lambda f=f: ocn.mask_immersed_field(f["c"]))
times = {k: [] for k in launches}
for r in range(rounds + 1):
    for k, (impl, fn) in launches.items():
        ocn.set_option("tendency_impl", impl)
        for _ in range(2):
            fn()
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            fn()
        ocn.synchronize()
        if r:
            times[k].append((time.perf_counter() - t0) / 10 * 1e3)
ocn.set_option("tendency_impl", 2)
for k, t in times.items():
    print(f"launch  {k:55s}: {med(t)} ms")
