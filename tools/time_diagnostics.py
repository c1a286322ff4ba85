"""On-device diagnostics at 256 x 256 x 128 with tanh-stretched z, (Periodic, Periodic, Bounded): the grid and model of
`bench.py --workload ppb_stretched` (GPU box). Device events on the library's stream, a warm-up, then `rounds` batches of REPS computes per
case; per case the time of one compute (median of the batches with their range) and the bytes per second it implies (every array read or
written once, 8 B per cell):
  Average(u, (1, 2)); Average(w*u, (1, 2)); Average(T); CumulativeIntegral(T, 3); Field(w*u); the five Langmuir profiles together
  (examples/langmuir_turbulence.jl:219-223: U, V, B, Average(w*u), Average(w*v), dims = (1, 2): seven arrays, 470 MB);
the five profiles again each time directly after a time-step (one event pair per sample, 50 samples) -- what a run pays: the step has
swept several GB through the caches, while back-to-back computes of one 67 MB array may be served by the 256 MiB Infinity Cache;
and in the same process the host route the five profiles replace (parent() copies + numpy) and one RK3 step of the model.
python tools/time_diagnostics.py [rounds = 5]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib
from helpers import smooth_state, tanh_faces

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 200
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

# ---- device events on the library's stream
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
    """ms per call of `run`, `reps` calls between two events"""
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


cells = N[0] * N[1] * N[2]
level = N[0] * N[1]
MB = lambda arrays, extra_levels=0: 8e-6 * (arrays * cells + extra_levels * level)      # noqa: E731
profiles = [ocn.Field(ocn.Average(x, dims=(1, 2))) for x in (u, v, T, w * u, w * v)]
cases = [("Average(u, (1, 2))", ocn.Field(ocn.Average(u, dims=(1, 2))), MB(1)),
         ("Average(w*u, (1, 2))", ocn.Field(ocn.Average(w * u, dims=(1, 2))), MB(2, 1)),
         ("Average(T)", ocn.Field(ocn.Average(T)), MB(1)),
         ("CumulativeIntegral(T, 3)", ocn.Field(ocn.CumulativeIntegral(T, dims=3)), MB(2)),
         ("Field(w*u)", ocn.Field(w * u), MB(3, 2))]
results = {}
print(f"{'case':34s} {'ms per compute (median [min, max])':38s} {'MB':>7s} {'TB/s':>6s}")
for name, field, mb in cases:
    med, lo, hi = timed(lambda field=field: ocn.compute(field))
    results[name] = med
    print(f"{name:34s} {med:8.4f} [{lo:.4f}, {hi:.4f}]{'':12s} {mb:7.1f} {mb / med * 1e-3:6.2f}")
mb = MB(7, 2)
med, lo, hi = timed(lambda: [ocn.compute(p) for p in profiles])
results["five profiles"] = med
print(f"{'five Langmuir profiles together':34s} {med:8.4f} [{lo:.4f}, {hi:.4f}]{'':12s} {mb:7.1f} {mb / med * 1e-3:6.2f}")

# ---- the five profiles directly after a step
after = []
for _ in range(55):
    ocn.time_step(model, dt)
    after.append(device_ms(lambda: [ocn.compute(p) for p in profiles], 1))
after = np.array(after[5:])
results["after a step"] = float(np.median(after))
print(f"{'five profiles, after a time-step':34s} {np.median(after):8.4f} [{after.min():.4f}, {after.max():.4f}]{'':12s} {mb:7.1f} {mb / np.median(after) * 1e-3:6.2f}")

# ---- the host route of the five profiles: parent() copies + numpy
H = model.grid.halo_size


def host_route():
    pu, pv, pw, pT = (x.parent() for x in (u, v, w, T))
    inner = lambda a, nz: a[H[0]:H[0] + N[0], H[1]:H[1] + N[1], H[2]:H[2] + nz]                   # noqa: E731
    out = [inner(a, N[2]).mean(axis=(0, 1)) for a in (pu, pv, pT)]
    for a, axis in ((pu, 0), (pv, 1)):
        lo = [slice(H[0], H[0] + N[0]), slice(H[1], H[1] + N[1]), slice(None)]
        hi = list(lo)
        hi[axis] = slice(H[axis] + 1, H[axis] + N[axis] + 1)
        ah = 0.5 * (a[tuple(lo)] + a[tuple(hi)])                                                   # ℑxᶜᵃᵃ / ℑyᵃᶜᵃ
        az = 0.5 * (ah[:, :, H[2] - 1:H[2] + N[2]] + ah[:, :, H[2]:H[2] + N[2] + 1])              # ℑzᵃᵃᶠ of it
        out.append((inner(pw, N[2] + 1) * az).mean(axis=(0, 1)))
    return out


host_route()
t = []
for _ in range(3):
    t0 = time.perf_counter()
    host = host_route()
    t.append((time.perf_counter() - t0) * 1e3)
print(f"{'host route (parent() + numpy)':34s} {np.median(t):8.1f} [{min(t):.1f}, {max(t):.1f}] ms")
for p, h in zip(profiles, host):
    ocn.compute(p)
    got = p.interior()[0, 0, :]
    assert np.allclose(got, h, rtol=1e-10, atol=1e-14), np.max(np.abs(got - h))

# ---- one RK3 step of the model
med, lo, hi = timed(lambda: ocn.time_step(model, dt), reps=10)
print(f"{'one RK3 step':34s} {med:8.4f} [{lo:.4f}, {hi:.4f}] ms")
print(f"five profiles / step = {100 * results['five profiles'] / med:.2f} % back to back, {100 * results['after a step'] / med:.2f} % after a step"
      f"   (host route = {np.median(t) / med:.1f} steps)")
