"""The draw of tests/physics_combinations.py covers what tests/test_gpu_physics_combinations.py is there for, and its yardstick composes
(CPU only; nothing here measures anything):
  * every feature is on in at least 3 of the 12 cases and off in at least 2;
  * every pair of features is on together in at least one case (the library accepts every pair of them; what it refuses -- a Flat z with a
    drift, the implicit discretisation on a Periodic z, conditions without walls -- is a matter of the grid, and is left out of the draw);
  * each of the four grids occurs (twice at least) and both timesteppers do; no drawn description is one the library refuses; the draw is reproducible;
  * the report keys expected of every description take each of their values somewhere;
  * ParticlesOrchestrated / StokesOrchestrated builds for every case from the oracle and takes one finite step."""
import itertools

import numpy as np
import pytest

import physics_combinations as PC


def coverage_failures(descriptions):
    """what the descriptions miss of the coverage conditions, as a list of sentences (empty: all hold)"""
    out = []
    feats = [PC.features(d) for d in descriptions]
    for f in PC.FEATURES:
        n_on = sum(x[f] for x in feats)
        if n_on < 3 or len(feats) - n_on < 2:
            out.append(f"{f} is on in {n_on} of {len(feats)} cases")
    for a, b in itertools.combinations(PC.FEATURES, 2):
        if not any(x[a] and x[b] for x in feats):
            out.append(f"{a} and {b} are never on together")
    for g in PC.GRIDS:
        if sum(d["grid"] == g for d in descriptions) < 2:
            out.append(f"grid {g} occurs in fewer than 2 cases")
    for t in PC.TIMESTEPPERS:
        if not any(d["timestepper"] == t for d in descriptions):
            out.append(f"timestepper {t} does not occur")
    for d in descriptions:
        out += [f"case {d['case']}: {r}" for r in PC.refusals(d)]
    return out


def test_the_draw_meets_the_coverage_conditions():
    descriptions = [PC.draw(c) for c in range(PC.N_CASES)]
    assert len(descriptions) == 12 and descriptions == [PC.draw(c) for c in range(PC.N_CASES)]
    assert coverage_failures(descriptions) == []
    assert all(max(PC.GRIDS[d["grid"]][1]) <= 10 for d in descriptions)
    # the conditions bite: a draw without its last four cases, or with one feature switched off everywhere, does not meet them
    assert coverage_failures(descriptions[:8])
    assert coverage_failures([dict(d, stokes=False) for d in descriptions])
    # a description the library refuses is named
    assert PC.refusals(dict(descriptions[0], grid="ppp", closure="scalar_vi", bcs=(("b", "top", "flux", 0.03),), halo=(3, 3, 7)))
    # every report key takes each of its values in some case: the plan's rules are exercised on both sides
    plans = [PC.expected_plan(d) for d in descriptions]
    assert {p["forcing_path"] for p in plans} == {0, 3} and {p["background_tendency_path"] for p in plans} == {0, 1, 2}
    assert {p["stokes_path"] for p in plans} == {0, 2} and {p["fuse_substep_active"] for p in plans} == {0, 1}
    assert {p["coriolis_kind"] for p in plans} == {0, 1, 2} and {p["tilted_gravity"] for p in plans} == {0, 1}
    assert {p["vertically_implicit"] for p in plans} == {0, 1} and {p["epilogue_march_active"] for p in plans} == {0, 1}
    assert all(PC.expected_plan(d, fused=False)["epilogue_march_active"] == 0 for d in descriptions)


@pytest.mark.parametrize("case", range(PC.N_CASES))
def test_the_yardstick_composes(oracle, case):
    """the chain Orchestrated -> Background -> Tilted -> Stokes -> Particles with the case's features on at once: one step on the CPU, every
    field, tendency and the pressure finite, the clock advanced, the particles moved and inside the domain"""
    import oldoceananigans_jl_amd as ocn
    d = PC.draw(case)
    grid = PC.make_grid(ocn, None, d)
    assert tuple(grid.halo_size) == d["halo"] and tuple(grid.size) == PC.GRIDS[d["grid"]][1]
    yard = PC.build_yardstick(ocn, oracle, d, grid)
    assert yard.g.H == d["halo"] and yard.g.N == PC.GRIDS[d["grid"]][1]
    start = {n: a.copy() for n, a in yard.P.items()} if d["particles"] else None
    dt = 0.05 / grid.Nx
    PC.step(yard, d, dt)
    for n in yard.names:
        assert np.all(np.isfinite(yard.U[n])) and np.all(np.isfinite(yard.Gn[n])) and np.all(np.isfinite(yard.Gm[n])), (case, n)
    assert np.all(np.isfinite(yard.p)) and yard.iteration == 1 and yard.time > 0.0
    if d["particles"]:
        assert yard.min_face_distance > 0.05 * min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ)
        assert any(not np.array_equal(yard.P[n], start[n]) for n in "xyz")
