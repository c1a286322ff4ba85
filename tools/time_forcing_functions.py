"""Relaxation with function masks and targets at 256 x 256 x 128 tanh-stretched (Periodic, Periodic, Bounded) -- the grid of bench.py
--workload ppb_stretched (GPU box): ms per RK3 step, medians of interleaved rounds of 10 steps with their range, device events on the
library's stream, of
  1. the unforced model;
  2. the built-in z-sponge (GaussianMask + LinearTarget) on all five fields, as the model chooses its path, and
  3. with fused_forcing = 0: the standalone table pass (add_forcing_kernel), the yardstick of the function form;
  4. the same sponge written as functions: tables + the per-cell program (forcing_function_hoist = 1), and
  5. the recorded program at every cell (forcing_function_hoist = 0);
  6. a fully mixed mask exp(-(x² + z²)) on all five fields, hoist 1, and 7. hoist 0;
  8. the sponge with a target that reads t: the refill launch before every tendency evaluation, no captured step.
On a build without the feature rows 1-3 only. `builtin` as a second argument builds rows 1-3 only on this build too: the like-for-like
A/B against the parent (the same three models resident): python tools/time_forcing_functions.py [rounds = 5] [builtin]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib, forcings
from helpers import smooth_state, tanh_faces

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
arch = ocn.GPU(0)
N = (256, 256, 128)
HAVE = hasattr(forcings, "refuse_functions_on_partitions") and "builtin" not in sys.argv[2:]
rate, zc, zw, T0, dTdz, omega = 1 / 60, -0.9, 0.1, 20.0, 0.01, 2 * np.pi / 3600

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


def make(sponge, options=()):
    grid = ocn.RectilinearGrid(arch, size=N, x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    forcing = None if sponge is None else {n: sponge for n in ("u", "v", "w", "T", "S")}
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), forcing=forcing)
    for key, value in options:
        model.set_option(key, value)
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 5))
    return model


table = ocn.Relaxation(rate=rate, mask=ocn.GaussianMask("z", center=zc, width=zw), target=ocn.LinearTarget("z", intercept=T0, gradient=dTdz))
rows = [("unforced", make(None)), ("built-in z-sponge, 5 fields", make(table)), ("built-in z-sponge, fused_forcing = 0", make(table, [("fused_forcing", 0)]))]
if HAVE:
    gaussian = lambda x, y, z: ocn.exp(-(z - zc) ** 2 / (2 * (zw * zw)))                                 # noqa: E731
    function = ocn.Relaxation(rate=rate, mask=gaussian, target=lambda x, y, z, t: T0 + dTdz * z)
    mixed = ocn.Relaxation(rate=rate, mask=lambda x, y, z: ocn.exp(-(x ** 2 + z ** 2)), target=lambda x, y, z, t: T0 + dTdz * z)
    moving = ocn.Relaxation(rate=rate, mask=gaussian, target=lambda x, y, z, t: T0 + dTdz * z + 0.5 * ocn.sin(omega * t))
    rows += [("z-sponge as functions, hoist 1", make(function)), ("z-sponge as functions, hoist 0", make(function, [("forcing_function_hoist", 0)])),
             ("mixed exp(-(x² + z²)) mask, hoist 1", make(mixed)), ("mixed exp(-(x² + z²)) mask, hoist 0", make(mixed, [("forcing_function_hoist", 0)])),
             ("z-sponge, target reads t", make(moving))]
dt, STEPS = 1e-4, 10
times = {name: [] for name, _ in rows}
for r in range(rounds + 1):                              # round 0 warms up
    for name, model in rows:
        ocn.synchronize()
        ms = device_ms(lambda: ocn.time_step(model, dt), STEPS)
        if r:
            times[name].append(ms)
for name, model in rows:
    extra = (f"functions {model.get_option('forcing_functions')}, per-cell instructions {model.get_option('forcing_function_cell_instructions')}, "
             if HAVE else "")
    print(f"{name:40s} ms/step {med(times[name])}   path {model.get_option('forcing_path')}, {extra}"
          f"finite {bool(np.isfinite(model.velocities.u.interior()).all())}")
base = np.median(times[rows[2][0]])
for name, _ in rows[3:]:
    d = np.median(times[name]) - base
    print(f"{name} - built-in standalone pass: {d * 1e3:+.1f} µs/step ({100 * d / base:+.3f} %)")
