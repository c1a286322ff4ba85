"""particles = LagrangianParticles at 256³ (triply periodic, the flagship workload of bench.py; GPU box): ms per RK3 step (medians of interleaved
rounds of 10 steps with their range) for n = 0 (particles = nothing), 10⁵, 10⁶ and 10⁷ random particles, and one launch of the particle
kernel on its own (ocn_advect_particles) with the bytes per second it achieves on the gathered lines: 24 corner loads of 8 bytes per
particle, each counted as the 64-byte line it touches (an upper bound on the traffic: neighbouring corners share lines), plus the
coalesced 48 bytes of x, y, z read and written. A build without the feature runs the n = 0 row only.
python tools/time_particles.py [rounds = 5] [largest n = 10000000]"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oldoceananigans_jl_amd as ocn
from helpers import smooth_state
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
largest = int(sys.argv[2]) if len(sys.argv) > 2 else 10 ** 7
arch = ocn.GPU(0)
N = 256
grid = ocn.RectilinearGrid(arch, size=(N, N, N), x=(0, 1), y=(0, 1), z=(0, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Periodic))
built = hasattr(ocn, "LagrangianParticles")
counts = [0] + ([n for n in (10 ** 5, 10 ** 6, 10 ** 7) if n <= largest] if built else [])


def med(t):
    t = np.array(t)
    return f"median {np.median(t):.3f}  range [{t.min():.3f}, {t.max():.3f}]"


rng = np.random.default_rng(1)
models, steps = {}, {}
for n in counts:
    lp = ocn.LagrangianParticles(x=rng.uniform(0, 1, n), y=rng.uniform(0, 1, n), z=rng.uniform(0, 1, n)) if n else None
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), **(dict(particles=lp) if built else {}))
    vals = smooth_state({k: grid.nodes(fl.loc) for k, fl in m.fields().items()}, 1234)
    ocn.set_model(m, **vals)
    models[n], steps[n] = m, []
step_dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6
for r in range(rounds + 1):                              # round 0 warms up
    for n, m in models.items():
        for _ in range(2):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ocn.time_step(m, step_dt)
        ocn.synchronize()
        if r:
            steps[n].append((time.perf_counter() - t0) / 10 * 1e3)
for n, t in steps.items():
    print(f"ms/step n = {n:>8d} particles (fuse_substep_active {models[n].get_option('fuse_substep_active')}): {med(t)}")

if built:
    m = models[0]
    u, v, w = m.velocities
    for n in counts[1:]:
        from oldoceananigans_jl_amd import _lib
        from oldoceananigans_jl_amd.kernels import _DeviceVectors
        d = _DeviceVectors([rng.uniform(0, 1, n) for _ in range(3)])
        launch = lambda: _lib.check(_lib.lib().ocn_advect_particles(grid.handle, n, *d.ptrs, None, 1.0, step_dt, u.data, v.data, w.data))   # noqa: E731
        times, REPS = [], 10
        for r in range(rounds + 1):
            for _ in range(2):
                launch()
            ocn.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                launch()
            ocn.synchronize()
            if r:
                times.append((time.perf_counter() - t0) / REPS * 1e3)
        ms = float(np.median(times))
        print(f"launch  particle_step_kernel n = {n:>8d}: {med(times)} ms; {n * (24 * 64 + 48) / (ms * 1e-3) / 1e9:.1f} GB/s on gathered 64-byte lines, "
              f"{n * (24 * 8 + 48) / (ms * 1e-3) / 1e9:.1f} GB/s on the bytes used")
        d.free()
