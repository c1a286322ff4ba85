"""Stencil-program diagnostics at 256 x 256 x 128 with tanh-stretched z, (Periodic, Periodic, Bounded): the grid and model of
tools/time_diagnostics.py after three steps (GPU box). Device events on the library's stream, a warm-up, then `rounds` batches of REPS
computes per case; per case the time of one compute (median of the batches with their range), the algorithmic bytes (every array read
or written once, 8 B per cell) and the bytes per second that implies:
  Field(ζ₃ᶠᶠᶜ); Average(w ∂z(T), (1, 2)); Average(ΣᵢⱼΣᵢⱼᶜᶜᶜ, (1, 2)); the kinetic-energy profile Average((u² + v² + w²) / 2 at ccc, (1, 2));
  Average(w * u, (1, 2)) once through the fixed evaluator and once through the interpreter -- what interpretation costs on identical work;
and in the same process the host route (parent() copies + numpy) for ζ and for ΣᵢⱼΣᵢⱼ.
python tools/time_stencil_diagnostics.py [rounds = 5]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib, diagnostics, operators as O
import stencil_reference as R
from helpers import smooth_state, tanh_faces

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 100
arch = ocn.GPU(0)
N = (256, 256, 128)
grid = ocn.RectilinearGrid(arch, size=N, x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N[2]), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
ocn.set_model(model, **smooth_state({n: model.grid.nodes(f.loc) for n, f in model.fields().items()}, 1234))
dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6
for _ in range(3):
    ocn.time_step(model, dt)
f = model.fields()
u, v, w, T = f["u"], f["v"], f["w"], f["T"]
Ce, Fa = ocn.Center, ocn.Face

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
    stream = C.c_void_p(_lib.lib().ocn_stream())
    assert hip.hipEventRecord(start, stream) == 0
    for _ in range(reps):
        run()
    assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
    return ms.value / reps


def timed(run, reps=REPS):
    for _ in range(5):
        run()
    ocn.synchronize()
    t = np.array([device_ms(run, reps) for _ in range(rounds)])
    return float(np.median(t)), float(t.min()), float(t.max())


cells, level = N[0] * N[1] * N[2], N[0] * N[1]
MB = lambda arrays, extra_levels=0: 8e-6 * (arrays * cells + extra_levels * level)      # noqa: E731
ζ = ocn.KernelFunctionOperation((Fa, Fa, Ce), O.ζ3ᶠᶠᶜ, grid, u, v)
Σ = ocn.KernelFunctionOperation((Ce, Ce, Ce), R.ΣᵢⱼΣᵢⱼᶜᶜᶜ, grid, u, v, w)
ke = ocn.KernelFunctionOperation((Ce, Ce, Ce), R.kinetic_energy_kernel, grid, u, v, w)
wu = w * u
wu_fixed, wu_interpreted = ocn.Field(ocn.Average(wu, dims=(1, 2))), ocn.Field(ocn.Average(wu, dims=(1, 2)))
cases = [("Field(ζ₃ᶠᶠᶜ)", lambda field=ocn.Field(ζ): ocn.compute(field), MB(3), ζ.stencil),
         ("Average(w ∂z(T), (1, 2))", lambda field=ocn.Field(ocn.Average(w * ocn.dz(T), dims=(1, 2))): ocn.compute(field), MB(2, 1), diagnostics.lower(w * ocn.dz(T))),
         ("Average(ΣᵢⱼΣᵢⱼᶜᶜᶜ, (1, 2))", lambda field=ocn.Field(ocn.Average(Σ, dims=(1, 2))): ocn.compute(field), MB(3, 1), Σ.stencil),
         ("kinetic-energy profile", lambda field=ocn.Field(ocn.Average(ke, dims=(1, 2))): ocn.compute(field), MB(3, 1), ke.stencil),
         ("Average(w*u, (1, 2)) fixed", lambda: ocn.compute(wu_fixed), MB(2, 1), None),
         ("Average(w*u, (1, 2)) interpreted", lambda: ocn.kernels.reduce_stencil(grid, wu, "average", (1, 2), False, False, wu_interpreted), MB(2, 1),
          diagnostics.lower(wu))]
print(f"{'case':36s} {'ins':>4s} {'slots':>5s} {'ms per compute (median [min, max])':38s} {'MB':>7s} {'TB/s':>6s}")
for name, run, mb, st in cases:
    med, lo, hi = timed(run)
    ins, slots = (len(st.program), st.nslots) if st is not None else (0, 0)
    print(f"{name:36s} {ins:4d} {slots:5d} {med:8.4f} [{lo:.4f}, {hi:.4f}]{'':12s} {mb:7.1f} {mb / med * 1e-3:6.2f}")
assert np.array_equal(wu_fixed.interior(), wu_interpreted.interior())

# ---- the host route: parent() copies + numpy
for name, host, device in (("ζ", lambda: R.vorticity(grid, u.parent(), v.parent()), ocn.Field(ζ)),
                           ("ΣᵢⱼΣᵢⱼ profile", lambda: R.strain(grid, u.parent(), v.parent(), w.parent()).mean(axis=(0, 1)), ocn.Field(ocn.Average(Σ, dims=(1, 2))))):
    host()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = host()
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"{'host route (parent() + numpy), ' + name:50s} {np.median(t):8.1f} [{min(t):.1f}, {max(t):.1f}] ms")
    got = device.interior()
    assert np.allclose(got.reshape(h.shape), h, rtol=1e-10, atol=1e-12)

med, lo, hi = timed(lambda: ocn.time_step(model, dt), reps=10)
print(f"{'one RK3 step':36s} {med:8.4f} [{lo:.4f}, {hi:.4f}] ms")
