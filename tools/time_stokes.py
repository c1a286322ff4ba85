"""stokes_drift = UniformStokesDrift at 256 x 256 x 128 with tanh-stretched z (GPU box), the `ppb_amd` physics of bench.py
(AnisotropicMinimumDissipation, linear SeawaterBuoyancy, the Flux / Gradient conditions): ms per RK3 step (medians of interleaved rounds of
10 steps with their range) of
  1. no drift: the marching epilogue -- the row to compare between two builds of the library;
  2. no drift with option epilogue_march = 0: the per-value epilogue without the Stokes terms;
  3. the drift on its default path: the per-value epilogue with the Stokes terms, the substep riding along;
  4. the drift with option fused_epilogue = 0: the stand-alone physics kernels, stokes_drift_kernel after them, the substep on its own --
     the nearest existing switch to "marching epilogue + stand-alone pass", which is priced in DESIGN.md and not built;
and the time of one stokes_drift_kernel launch. A build without the feature runs row 1 only.
python tools/time_stokes.py [rounds = 5]"""
import sys, os, time, math
import ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib
from helpers import smooth_state, tanh_faces
sys.path.insert(0, ROOT)
from bench import workload_physics
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0, 1), y=(0, 1), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
built = hasattr(ocn, "UniformStokesDrift")


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]"


drift = None
if built:
    # the Langmuir example's shape: an exponential shear, decay scale a tenth of the depth
    drift = ocn.UniformStokesDrift(dz_us=lambda z, t: 0.07 * math.exp(z / 0.1))
    # ---- one launch of the stand-alone kernel: device tables made once, REPS launches per timing
    L = _lib.lib()
    tables = drift.tables(grid)
    block = C.c_void_p()
    _lib.check(L.ocn_malloc(C.byref(block), sum(t.nbytes for t in tables)))
    ptrs, off = [], 0
    for t in tables:
        ptrs.append(C.c_void_p(block.value + off))
        _lib.check(L.ocn_memcpy_h2d(ptrs[-1], t.ctypes.data_as(C.c_void_p), t.nbytes))
        off += t.nbytes
    rng = np.random.default_rng(1)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    f = {n: make[n](grid) for n in "uvw"}
    G = {n: make[n](grid) for n in "uvw"}
    for a in f.values():
        a.set_parent(rng.standard_normal(a.shape))
    launch = lambda: _lib.check(L.ocn_add_stokes_drift(grid.handle, *ptrs, f["u"].data, f["v"].data, f["w"].data, G["u"].data, G["v"].data,   # noqa: E731
                                                       G["w"].data, None, None, None))
    times, REPS = [], 10
    for r in range(rounds + 1):                          # round 0 warms up
        for _ in range(2):
            launch()
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            launch()
        ocn.synchronize()
        if r:
            times.append((time.perf_counter() - t0) / REPS * 1e3)
    print(f"launch  stokes_drift_kernel (u, v, w): {med(times)} ms")
    _lib.check(L.ocn_free(block))
    del f, G

# ---- ms per step
variants = {"1 no drift (marching epilogue)": (False, {})}
if built:
    variants.update({"2 no drift, epilogue_march = 0": (False, {"epilogue_march": 0}),
                     "3 drift, per-value epilogue (default)": (True, {}),
                     "4 drift, fused_epilogue = 0": (True, {"fused_epilogue": 0})})
models, steps = {}, {}
for name, (with_drift, options) in variants.items():
    kw = dict(stokes_drift=drift) if with_drift else {}
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), **workload_physics(ocn, "ppb_amd"), **kw)
    for k, v in options.items():
        m.set_option(k, v)
    vals = smooth_state({n: grid.nodes(fl.loc) for n, fl in m.fields().items()}, 1234)
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
    report = ", ".join(f"{k} {m.get_option(k)}" for k in (("stokes_path",) if built else ()) + ("epilogue_march_active", "fuse_substep_active"))
    print(f"ms/step {name:40s} ({report}): {med(t)}")
