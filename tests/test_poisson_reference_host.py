"""The long-double Poisson reference (poisson_reference.py) certifies itself on every white-noise case of poisson_cases.py, and the CPU oracle's
solve is measured against it: this is where the oracle's own error at each shape is written down (printed, recorded as test properties, and
tabulated in DESIGN.md). No GPU."""
import numpy as np
import pytest

import poisson_reference as PR
from poisson_cases import (MODEL_CASES, SOLVER_CASES, assert_same_metrics, case_id, oracle_grid, oracle_projection, seed_of, white_noise_parents,
                           z_faces_of)

EPS = PR.EPS


@pytest.mark.parametrize("case", SOLVER_CASES, ids=case_id)
def test_oracle_solve_against_long_double(oracle, case, record_property):
    geom = PR.Geometry(case.size, case.topology, z_faces_of(case))
    g_cpu = oracle_grid(oracle, case)
    assert geom.H == g_cpu.H
    assert_same_metrics(geom, g_cpu.dc[2], g_cpu.df[2], g_cpu.H[2])
    for d, h in ((0, geom.dx), (1, geom.dy)):
        assert case.topology[d] == "Flat" or float(h) == g_cpu.dc[d][0]
    A = white_noise_parents(oracle, g_cpu, seed_of(case))
    weighted = case.kind == 1
    R = PR.source_term(geom, *A, weighted)
    p_ref = PR.solve(R, geom, weighted)
    res = PR.certify(p_ref, R, geom, weighted)
    # the oracle: its own float64 source term of the same velocities, its own transforms
    s_cpu = oracle.PoissonSolver(g_cpu, case.kind)
    rhs = g_cpu.source_term(*A, weight_by_dz=weighted)
    assert PR.rel_err(rhs.real, R) <= 64 * EPS           # one divergence: a few roundings of O(N) terms against max |R|
    s_cpu.rhs[...] = rhs
    p_cpu = g_cpu.zeros(oracle.LOC["c"])
    s_cpu.solve(p_cpu)
    p_oracle = g_cpu.interior_cells(p_cpu)
    err = PR.rel_err(p_oracle, p_ref)
    cond = PR.condition_estimate(geom)
    res_oracle = PR.relative_residual(p_oracle, R, geom, weighted)
    mean = abs(float(np.mean(p_oracle, dtype=PR.LD))) / (EPS * np.abs(p_oracle).max())
    print(f"{case_id(case):48s} long-double residual {res:.1e}  oracle error {err:.1e}  error / (eps cond) {err / (EPS * cond):.3f}  "
          f"oracle residual {res_oracle:.1e}  |mean| / (eps max|p|) {mean:.2f}")
    record_property("long_double_residual", res)
    record_property("oracle_error", err)
    record_property("oracle_error_over_eps_cond", err / (EPS * cond))
    assert err <= 4 * EPS * cond, (err, cond)


@pytest.mark.parametrize("case", MODEL_CASES, ids=case_id)
def test_oracle_projection_against_long_double(oracle, case, record_property):
    """set!(model; enforce_incompressibility = true) of the oracle model on white noise: the projected velocities against u - ∂p of the
    long-double solve, and their divergence evaluated in long double"""
    geom = PR.Geometry(case.size, case.topology, z_faces_of(case))
    g_cpu = oracle_grid(oracle, case)
    out = oracle_projection(oracle, g_cpu, geom, case)
    for n in "uvw":
        print(f"{case_id(case):36s} {n}: oracle error {out['err'][n]:.1e}")
        record_property("oracle_error_" + n, out["err"][n])
        assert out["err"][n] <= 4 * EPS * PR.condition_estimate(geom)
    print(f"{case_id(case):36s} max |div u| / max |div u0|: oracle {out['div']:.1e}, long double {out['div_ref']:.1e}")
    record_property("oracle_divergence", out["div"])
    assert out["div_ref"] <= 1e-15
