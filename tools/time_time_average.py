"""One iteration's advance of time-averaged diagnostics at 256 x 256 x 128 with tanh-stretched z, (Periodic, Periodic, Bounded): the grid
and model of `bench.py --workload ppb_stretched` (GPU box). Two routes per case, on the same build:
  folded        the integrand is formed and folded into the running average in one pass (ocn_time_average_*: the fold at the store of
                the diagnostics kernels), what WindowedTimeAverage(operation or scan) does;
  materialised  ocn.compute into a Field (for a full-size operation with its halo fill), then the fold of that field as a plain operand:
                what WindowedTimeAverage(Field(...)) does, and all a caller had before the store-site fold.
Cases: (a) the five Langmuir profiles (examples/langmuir_turbulence.jl:219-223: U, V, B, Average(w*u), Average(w*v), dims = (1, 2));
(b) one full-size w * T -- folded: read w, T, result, write result (4 arrays); materialised: 6 arrays and a halo fill.
Device events on the library's stream, a warm-up, then `rounds` rounds in which the two routes ALTERNATE, REPS advances per batch: per
route the median of the batches with their range. Then the same directly after a time-step (one event pair per sample, the routes
alternating from step to step): what a run pays, with the caches swept by the step. Last, one RK3 step of the model for scale.
The results of the two routes are compared bit for bit before anything is timed.
python tools/time_time_average.py [rounds = 5]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import _lib, time_averages
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


# a sample in the middle of a window: weights 1/3 and 2/3, so repeated advances stay bounded
TIMES = (0.5, 1.0, 1.5, False)
schedule = ocn.AveragedTimeInterval(4.0, window=2.5)


class Folded:
    """the in-flight route of a list of operands"""

    def __init__(self, operands):
        self.wtas = [ocn.WindowedTimeAverage(op, model, schedule=schedule.copy()) for op in operands]

    def advance(self):
        for wta in self.wtas:
            time_averages.accumulate_result(wta, TIMES)

    def results(self):
        return [wta.result.interior() for wta in self.wtas]


class Materialised:
    """compute into a Field (with its halo fill, for an operation), then fold that field as a plain operand"""

    def __init__(self, operands):
        self.fields = [ocn.Field(op) for op in operands]
        self.results_ = [ocn.Field(x.loc, grid) for x in self.fields]
        for x, r in zip(self.fields, self.results_):
            r.set_parent(x.parent())

    def advance(self):
        for x, r in zip(self.fields, self.results_):
            ocn.compute(x)
            if None in x.loc:                                # a reduced field has no operand form: its whole (small) parent
                ocn.kernels.time_average_parent(x, TIMES, r)
            else:
                ocn.kernels.time_average_operation(grid, x, TIMES, r)

    def results(self):
        return [r.interior() for r in self.results_]


rows = N[1]                                                 # (j, k) rows per output element of Average(·, dims=(1, 2)): one level
chunks = -(-rows // 16)                                      # DG_ROWS = 16: more than one chunk means a second, combining launch
reduce_launches = 2 if chunks > 1 else 1
profiles = [ocn.Average(x, dims=(1, 2)) for x in (u, v, T, w * u, w * v)]
cases = [("(a) five Langmuir profiles", profiles, 5 * reduce_launches, 5 * (reduce_launches + 1)),
         ("(b) full-size w * T", [w * T], 1, 3)]              # materialised (b): compute, halo fill, fold
step = lambda: ocn.time_step(model, dt)                      # noqa: E731

print(f"{'case':30s} {'route':13s} {'launches':>8s}  {'ms per advance, back to back':34s} {'ms per advance, after a step':34s}")
summary = {}
for name, operands, n_folded, n_materialised in cases:
    routes = [("folded", Folded(operands), n_folded), ("materialised", Materialised(operands), n_materialised)]
    # the two routes hold the same bits before and after an advance
    for _ in range(2):
        a, b = (r.results() for _, r, _ in routes)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        for _, r, _ in routes:
            r.advance()
    for _, r, _ in routes:                                   # warm-up of every shape timed
        for _ in range(5):
            r.advance()
    ocn.synchronize()
    back = {label: [] for label, _, _ in routes}
    for _ in range(rounds):                                  # alternate the routes inside every round
        for label, r, _ in routes:
            back[label].append(device_ms(r.advance, REPS))
    after = {label: [] for label, _, _ in routes}
    for s in range(2 * 25 + 4):
        step()
        label, r, _ = routes[s % 2]
        ms = device_ms(r.advance, 1)
        if s >= 4:
            after[label].append(ms)
    for label, r, launches in routes:
        b, a = np.array(back[label]), np.array(after[label])
        summary[(name, label)] = (float(np.median(b)), float(np.median(a)))
        print(f"{name:30s} {label:13s} {launches:8d}  {np.median(b):8.4f} [{b.min():.4f}, {b.max():.4f}]{'':8s} {np.median(a):8.4f} [{a.min():.4f}, {a.max():.4f}]")

for _ in range(3):
    step()
ocn.synchronize()
t = np.array([device_ms(step, 10) for _ in range(rounds)])
rk3 = float(np.median(t))
print(f"{'one RK3 step':30s} {'':13s} {'':8s}  {rk3:8.4f} [{t.min():.4f}, {t.max():.4f}]")
for name, _, _, _ in cases:
    fb, fa = summary[(name, "folded")]
    mb, ma = summary[(name, "materialised")]
    print(f"{name}: folded / materialised = {fb / mb:.3f} back to back, {fa / ma:.3f} after a step; folded = {100 * fa / rk3:.2f} % of a step (after a step)")
