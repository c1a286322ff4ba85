"""The recorded states of test_gpu_pressure_step_kernels.py (tests/golden/pressure_step_*.npy) against the CPU oracle: the yardstick must
itself be right. Every case is one RK3 step of the oracle's model on the same grid from the same state -- a one-rank slab that is its own
neighbour is the serial model on its global grid. helpers.rel_err < 1e-12 on the interiors, pNHS with the error model of
test_gpu_option_variants.py, as test_gpu_folded_pressure_step.py asserts it. No GPU."""
import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn
from dist_worker import analytic
from helpers import ORACLE_TOPO, rel_err, smooth_state, tanh_faces
from pressure_step_cases import CASES, case_id, golden_path, time_step_of, unpack

TOPOLOGY = {"P": "Periodic", "B": "Bounded", "F": "Flat"}
CNAMES = ["u", "v", "w", "c0", "c1"]


def _oracle_step(oracle, case):
    """-> ({name: the oracle's parent array after the step}, the host grid)"""
    names = [TOPOLOGY[t] for t in case.topology]
    z = (0.0, 1.0) if case.topology[2] == "P" else (tanh_faces(case.size[2]) if case.z == "stretched" else (-1.0, 0.0))
    x = (0.0, 2.0) if case.kind == "slab" else (0.0, 1.0)
    topology = tuple(getattr(ocn, n) for n in names)
    if "F" in case.topology:
        grid = ocn.RectilinearGrid(None, size=(case.size[0], case.size[2]), x=x, z=z, topology=topology)
    else:
        grid = ocn.RectilinearGrid(None, size=case.size, x=x, y=(0.0, 1.0), z=z, topology=topology)
    g_cpu = oracle.Grid(case.size, topology=tuple(ORACLE_TOPO[n] for n in names), x=x, y=(0.0, 1.0), z=z)
    m_cpu = oracle.Model(g_cpu, len(case.tracers))
    F, Cc = ocn.Face, ocn.Center
    locs = {"u": (F, Cc, Cc), "v": (Cc, F, Cc), "w": (Cc, Cc, F)} | {t: (Cc, Cc, Cc) for t in case.tracers}
    if case.kind == "single":
        vals = smooth_state({n: grid.nodes(loc) for n, loc in locs.items()}, 1234)
    else:
        vals = {n: analytic(n, *grid.nodes(loc)) for n, loc in locs.items()}
    m_cpu.set(**{cn: vals[n] for cn, n in zip(CNAMES, locs)})
    m_cpu.time_step(time_step_of(case))
    out = {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, locs)}
    out["pNHS"] = m_cpu.field("p").copy()
    return out, grid


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_recorded_state_is_the_oracles(oracle, case):
    ref, grid = _oracle_step(oracle, case)
    core = tuple(slice(3, -3) if t != "F" else slice(None) for t in case.topology)
    if case.kind == "slab":
        ref = {n: ref[n][core] for n in ("u", "v", "w", "pNHS")}
    got = unpack(np.load(golden_path(case)), ref)
    if case.kind == "single":
        got, ref = {n: a[core] for n, a in got.items()}, {n: a[core] for n, a in ref.items()}
    dt = time_step_of(case)
    umax = max(np.abs(ref[n]).max() for n in ("u", "v", "w"))
    dmax = max(d for d, t in zip((grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.max(grid.Δzᵃᵃᶜ))), case.topology) if t != "F")
    for n, a in got.items():
        if n == "pNHS":          # p = lap^-1(div u*) / dt carries the velocities' round-off times dx / dt
            pscale = max(np.abs(ref[n]).max(), umax * dmax / dt)
            err = np.max(np.abs(a - ref[n]))
            print(case_id(case), n, "abs err", err, "bound", 1e-12 * pscale)
            assert err < 1e-12 * pscale, (n, err, pscale)
            continue
        print(case_id(case), n, "rel err", rel_err(a, ref[n]))
        assert rel_err(a, ref[n]) < 1e-12, (n, rel_err(a, ref[n]))
