"""Function-valued Flux conditions at 256 x 256 x 128 tanh-stretched (Periodic, Periodic, Bounded) with ScalarDiffusivity -- the grid of
bench.py --workload ppb_stretched (GPU box): ms per RK3 step, medians of interleaved rounds of 10 steps with their range, device events
on the library's stream, of
  1. constant array-valued Flux conditions on the bottom of u and v and on the top of T: the model as it was before functions existed;
  2. the quadratic drag -cD sqrt(u² + v²) u / v on the bottom of u and v and Q(t) = Q₀ sin(ωt) on the top of T as functions: one
     evaluation launch before each of the three uses of the Flux conditions in a step, and (Q reads t) no replay of a captured step;
  3. the two drags alone (no t): the same launches, the captured step kept where option use_graph asks for one;
and the evaluation launch on its own through ocn_evaluate_boundary_function (enqueued back to back, device events).
On a build without the feature row 1 only, for A/B against the parent: python tools/time_boundary_functions.py [rounds = 5]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib
from helpers import smooth_state, tanh_faces

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)
HAVE = hasattr(ocn, "ContinuousBoundaryFunction")
cD, Q0, omega = 2.5e-3, 1e-4, 2 * np.pi / 86400

try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
start, stop = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0


def device_ms(run, reps):
    """ms per call of `run`, `reps` calls between two events on the library's stream"""
    stream = C.c_void_p(_lib.lib().ocn_stream())
    assert hip.hipEventRecord(start, stream) == 0
    for _ in range(reps):
        run()
    assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
    return ms.value / reps


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.4f}  range [{t.min():.4f}, {t.max():.4f}]"


def make(kind):
    grid = ocn.RectilinearGrid(arch, size=N, x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    F, Flux = ocn.FieldBoundaryConditions, ocn.FluxBoundaryCondition
    if kind == "arrays":
        rng = np.random.default_rng(3)
        bcs = {"u": F(bottom=Flux(1e-5 * rng.standard_normal(N[:2]))), "v": F(bottom=Flux(1e-5 * rng.standard_normal(N[:2]))),
               "T": F(top=Flux(Q0 * rng.standard_normal(N[:2])))}
    else:
        bcs = {"u": F(bottom=Flux(lambda x, y, t, u, v, p: -p * ocn.sqrt(u ** 2 + v ** 2) * u, field_dependencies=("u", "v"), parameters=cD)),
               "v": F(bottom=Flux(lambda x, y, t, u, v, p: -p * ocn.sqrt(u ** 2 + v ** 2) * v, field_dependencies=("u", "v"), parameters=cD))}
        if kind == "functions":
            bcs["T"] = F(top=Flux(lambda x, y, t: Q0 * ocn.sin(omega * t)))
        else:
            bcs["T"] = F(top=Flux(Q0 * np.random.default_rng(3).standard_normal(N[:2])))
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.ScalarDiffusivity(ν=1e-4, κ=1e-4), boundary_conditions=bcs)
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 5))
    return model


rows = [("array-valued Flux conditions (3 sides)", make("arrays"))]
if HAVE:
    rows += [("drag on u, v + Q0 sin(wt) on T as functions", make("functions")), ("drag on u, v as functions (no t)", make("drag"))]
dt, STEPS = 1e-4, 10
times = {name: [] for name, _ in rows}
for r in range(rounds + 1):                              # round 0 warms up
    for name, model in rows:
        ocn.synchronize()
        ms = device_ms(lambda: ocn.time_step(model, dt), STEPS)
        if r:
            times[name].append(ms)
for name, model in rows:
    extra = f"functions {model.get_option('boundary_functions')}, launches per use {model.get_option('boundary_function_launches')}, " if HAVE else ""
    print(f"{name:45s} ms/step {med(times[name])}   {extra}graph replays {model.get_option('graph_replays')}, "
          f"finite {bool(np.isfinite(model.velocities.u.interior()).all())}")
if HAVE:
    base = np.median(times[rows[0][0]])
    for name, _ in rows[1:]:
        d = np.median(times[name]) - base
        print(f"{name} - arrays: {d * 1e3:+.1f} µs/step ({100 * d / base:+.3f} %)")
    # ---- the evaluation launch on its own: the drag of u over 256 x 256 points
    from oldoceananigans_jl_amd.boundary_functions import assumed_field_location, trace
    model = rows[1][1]
    f = model.fields()
    program = trace(lambda x, y, t, u, v: -cD * ocn.sqrt(u ** 2 + v ** 2) * u, [0, 1], 2)
    out = ocn.CenterField(model.grid)
    run = lambda: ocn.kernels.evaluate_boundary_function(model.grid, program, assumed_field_location("u"), "bottom", [f["u"], f["v"]], 0.0, out=out.data)   # noqa: E731
    run()
    t = [device_ms(run, 50) * 1e3 for _ in range(rounds)]
    print(f"ocn_evaluate_boundary_function, drag of u, 256 x 256 points (launch + its table upload and synchronisation): µs {med(t)}")
