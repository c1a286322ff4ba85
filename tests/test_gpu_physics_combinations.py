"""Models with several recent features on at once, against the composed yardstick (tests/physics_combinations.py draws the 12 seeded
descriptions; tests/test_physics_combinations_host.py holds the draw to its coverage conditions): BackgroundField, gravity_unit_vector and
ConstantCartesianCoriolis, UniformStokesDrift, the vertically implicit ScalarDiffusivity, array forcing, Flux / Value conditions and
LagrangianParticles, on four grids at several halos with RK3 and AB2. plan() decides the forcing path, the background path, fuse_substep
and stokes_path from all of them together; each per-feature file pins its feature alone or with one fixed companion set.

Per case, two steps at Δt = 0.05 / Nx from the same projected helpers.smooth_state:
  * the report keys answer the rules of include/ocn_mi355x.h for the description (physics_combinations.expected_plan);
  * u, v, w and the tracers over the interior: rel_err < 1e-12 against ParticlesOrchestrated (StokesOrchestrated without particles); the
    pressure to 1e-12 of the scale of test_gpu_stokes.test_model_is_the_orchestrated_yardstick; the clock ==; particle positions to 1e-12 of
    the domain length (test_gpu_particles.py) after the yardstick has shown that none came within 1e-6 of a face -- the tolerances the
    per-feature files use, none of them new. The measured worst values are printed (DESIGN.md 30 records them);
  * a second model with fused_epilogue = 0 and fuse_substep = 0 -- the stand-alone physics kernels, stokes_drift_kernel, the substep as its
    own launch -- is np.array_equal to the default one in fields, Gⁿ, G⁻, pNHS and particle positions."""
import numpy as np
import pytest

from helpers import rel_err
import halo_cases as HC
import particles_reference as P
import physics_combinations as PC

pytestmark = pytest.mark.gpu

STEPS = 2
PLAN_KEYS = ("forcing_path", "background_tendency_path", "stokes_path", "fuse_substep_active", "epilogue_march_active", "coriolis_kind",
             "tilted_gravity", "vertically_implicit")


def _case_id(case):
    d = PC.draw(case)
    return f"{case}-{d['grid']}-{'rk3' if d['timestepper'] == 'RungeKutta3' else 'ab2'}"


@pytest.mark.parametrize("case", range(PC.N_CASES), ids=_case_id)
def test_model_is_the_composed_yardstick(ocn, oracle, arch, case):
    d = PC.draw(case)
    assert not PC.refusals(d)
    grid, model = PC.build_model(ocn, arch, d)
    _, plain = PC.build_model(ocn, arch, d, options={"fused_epilogue": 0, "fuse_substep": 0})
    yard = PC.build_yardstick(ocn, oracle, d, grid)
    assert tuple(grid.halo_size) == d["halo"] == yard.g.H
    for m, fused in ((model, True), (plain, False)):
        got = {k: m.get_option(k) for k in PLAN_KEYS}
        assert got == PC.expected_plan(d, fused), (case, fused, d)
        assert m.get_option("stokes_drift") == int(d["stokes"]) and m.get_option("background_fields") == len(d["background"])
        assert m.get_option("particles") == len(d["particles"])
    dt = 0.05 / grid.Nx
    for _ in range(STEPS):
        ocn.time_step(model, dt)
        ocn.time_step(plain, dt)
        PC.step(yard, d, dt)
    locs = PC.locations(ocn, d)
    worst = 0.0
    for gn in model.fields():
        cn = PC.yard_name(d, gn)
        a, b = HC.interior(grid, model.fields()[gn].parent(), locs[gn]), HC.interior(grid, yard.U[cn], locs[gn])
        assert np.all(np.isfinite(a))
        worst = max(worst, rel_err(a, b))
        assert rel_err(a, b) < 1e-12, (case, gn, rel_err(a, b))
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    a, b = HC.interior(grid, model.pressures.pNHS.parent()), HC.interior(grid, yard.p)
    pscale = max(np.abs(b).max(), umax * max(s for s, t in zip((grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ), grid.topology) if t is not ocn.Flat) / dt)
    perr = np.max(np.abs(a - b)) / pscale
    assert perr < 1e-12, (case, perr)
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == STEPS
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    xerr = 0.0
    if d["particles"]:
        g = yard.geometry
        assert yard.min_face_distance > 1e-6, yard.min_face_distance
        start = PC.particle_positions(g, d)
        for k, n in enumerate("xyz"):
            got, want = getattr(model.particles, n), yard.P[n]
            L = g.length(k) if g.topo[k] != P.FLAT else 1.0
            xerr = max(xerr, np.abs(got - want).max() / L)
            assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-12 * L, (case, n, np.abs(got - want).max())
        assert np.abs(model.particles.x - start[0]).max() > 1e-4               # they moved, by far more than the tolerance
    print(f"case {case} {d['grid']} {d['timestepper']}: worst field rel_err {worst:.3e}, pressure {perr:.3e} of its scale, particles {xerr:.3e} of the length")
    # the unfused arm: the same bits
    for n in model.fields():
        for label, get in (("field", lambda m: m.fields()[n]), ("Gn", lambda m: m.tendency(n)), ("Gm", lambda m: m.tendency(n, previous=True))):
            a, b = get(plain).parent(), get(model).parent()
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (case, label, n, np.abs(a - b).max())
    assert np.array_equal(plain.pressures.pNHS.parent(), model.pressures.pNHS.parent()), case
    for n in "xyz" if d["particles"] else "":
        assert np.array_equal(getattr(plain.particles, n), getattr(model.particles, n)), (case, n)
    model.close()
    plain.close()
