"""OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)) and the mass-flux correction on the MI355X against the numpy
restatement (tests/open_boundary_reference.py, pinned on the CPU by tests/test_open_boundary_host.py):
  * the boundary step on its own, `==` the restatement: every side, constant and array value, both signs of ū;
  * the flux integral and the correction on their own, within the round-off bound of the sums, identical bits on a second call;
  * the model (3 RK3 and 3 AB2 steps) against the orchestrated yardstick, 1e-12;
  * the reference's mass-conservation and relaxation tests (test/test_boundary_conditions_integration.jl:145-182, 370-386);
  * a model with imposed open conditions only is what it was: same bits, no added launch."""

import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import open_boundary_reference as R
from vertically_implicit_reference import EPS, Metrics

pytestmark = pytest.mark.gpu
INF = float("inf")

# (9, 20, 13): faces of 260, 117 and 180 points -- more than one 256-thread block, none a multiple of 64; (66, 16): a slice with a Flat y
GRIDS = {"bbb_stretched": dict(size=(9, 20, 13), topo="BBB", stretched=True), "slice": dict(size=(66, 16), topo="BFB", stretched=False)}


def _grid(ocn, arch, name):
    c = GRIDS[name]
    topo = tuple({"P": ocn.Periodic, "B": ocn.Bounded, "F": ocn.Flat}[t] for t in c["topo"])
    kw = dict(z=tanh_faces(c["size"][-1]) if c["stretched"] else (-1.0, 0.0), x=(0.0, 1.0))
    if topo[1] is not ocn.Flat:
        kw["y"] = (0.0, 2.0)
    return ocn.RectilinearGrid(arch, size=c["size"], topology=topo, **kw)


def _sides(m):
    return [s for s in R.SIDES if m.topo[R.SIDES.index(s) // 2] == 1]


def _random_velocities(ocn, grid, seed):
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds, parents = {}, {}
    for n in "uvw":
        f = make[n](grid)
        a = np.asfortranarray(0.5 + rng.standard_normal(f.shape))
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


def _face_shape(m, side):
    d = R.SIDES.index(side) // 2
    return tuple(m.N[q] for q in range(3) if q != d)


@pytest.mark.parametrize("name", list(GRIDS))
def test_boundary_step_is_the_restatement_bit_for_bit(ocn, arch, name):
    grid = _grid(ocn, arch, name)
    m = Metrics.of_grid(grid)
    rng = np.random.default_rng(7)
    # Δt / ΔX ū on both sides of the clamps at 0 and ±1, both timescales finite, zero and infinite, last_stage_Δt = Inf
    cases = [(0.3, 2.0, 0.02), (0.0, INF, 0.02), (0.5, 0.0, 0.3), (0.3, 2.0, INF)]
    for side in _sides(m):
        n = R.NORMAL[side]
        values = [1.3, -0.7, 0.0, np.asfortranarray(rng.standard_normal(_face_shape(m, side)) * 3.0)]       # the array: both signs point by point
        for tin, tout, dt in cases:
            for value in values:
                flds, P = _random_velocities(ocn, grid, 11)
                want = R.step_side(m, P[n].copy(order="F"), side, value, tin, tout, dt)
                bc = ocn.OpenBoundaryCondition(value, scheme=ocn.PerturbationAdvection(tin, tout))
                ocn.kernels.step_open_boundary(flds[n], side, bc, dt)
                got = flds[n].parent()
                assert np.array_equal(got, want), (side, tin, tout, dt, np.abs(got - want).max())
                if isinstance(value, np.ndarray) and not np.isinf(dt):
                    assert not np.array_equal(got, P[n]), (side, tin, tout, dt)


def test_boundary_step_refusals(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    grid = ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1), topology=(ocn.Bounded, ocn.Periodic, ocn.Bounded))
    u, v, c = ocn.XFaceField(grid), ocn.YFaceField(grid), ocn.CenterField(grid)
    call = lambda f, side, tin=0.0, tout=INF: L.ocn_step_open_boundary(grid.handle, f.data, _lib.i3(f.loc_codes), side, 1.0, None, tin, tout, 0.1)   # noqa: E731
    assert call(u, 0) == 0 and call(u, 1) == 0
    assert call(u, 4) == -1 and call(c, 0) == -1 and call(v, 2) == -1 and call(u, 6) == -1          # not wall-normal; Center; Periodic y; no such side
    assert call(u, 0, -1.0) == -1 and call(u, 0, 0.0, float("nan")) == -1
    # the model setter: OCN_EINVAL = -1 where the reference has no method, and for a side whose condition is not Open
    model = ocn.NonhydrostaticModel(grid=grid, boundary_conditions={"u": ocn.FieldBoundaryConditions(west=ocn.OpenBoundaryCondition(1.0))})
    setter = lambda name, side, on=1: L.ocn_model_set_open_boundary_scheme(model.handle, name, side, on, 0.0, INF)         # noqa: E731
    assert setter(b"c0", 0) == -1 and setter(b"u", 4) == -1 and setter(b"v", 2) == -1 and setter(b"w", 0) == -1
    assert setter(b"u", 1) == -1 and b"Open" in L.ocn_last_error()                                   # east is the default wall
    assert model.get_option("open_boundary_scheme_sides") == 0
    assert setter(b"u", 0) == 0 and model.get_option("open_boundary_scheme_sides") == 1 and model.get_option("open_boundary_launches") == 3
    assert setter(b"u", 0, 0) == 0 and model.get_option("open_boundary_scheme_sides") == 0 and model.get_option("open_boundary_launches") == 0
    model.close()


@pytest.mark.parametrize("name", list(GRIDS))
def test_flux_integral_and_correction(ocn, arch, name):
    grid = _grid(ocn, arch, name)
    m = Metrics.of_grid(grid)
    sides = _sides(m)
    flds, P = _random_velocities(ocn, grid, 13)
    u, v, w = flds["u"], flds["v"], flds["w"]
    # the integral: every face on its own, then all of them
    for subset in [[s] for s in sides] + [sides]:
        conditions = {s: np.zeros(_face_shape(m, s)) for s in subset}            # "integrate this face"
        want = R.mass_inflow(m, P, conditions, {})
        bound = R.flux_bound(m, P, conditions, {})
        got = ocn.kernels.open_boundary_mass_inflow(grid, u, v, w, subset)
        print(subset, "inflow", got, "restatement", want, "bound", bound)
        assert abs(got - want) <= bound and abs(want) > 100 * bound
        assert ocn.kernels.open_boundary_mass_inflow(grid, u, v, w, subset) == got                   # a fixed summation order
    assert ocn.kernels.open_boundary_mass_inflow(grid, u, v, w, []) == 0.0
    # the correction: scheme faces, an array-valued and a constant imposed face, a default wall
    rng = np.random.default_rng(17)
    pa = ocn.PerturbationAdvection(0.1, INF)
    arr = np.asfortranarray(rng.standard_normal(_face_shape(m, "top")))
    cases = [{s: (0.4, True) for s in sides},
             {"west": (1.0, False), "east": (1.0, True)},
             {"west": (0.8, True), "bottom": (-0.3, False), "top": (arr, False)},
             {"east": (0.0, True), "bottom": (0.1, True), "top": (arr, True)}]
    for case in cases:
        conditions = {s: c for s, (c, _) in case.items()}
        schemes = {s: (0.1, INF) for s, (_, on) in case.items() if on}
        start = {n: a.copy(order="F") for n, a in P.items()}
        for s, (c, on) in case.items():                                          # an imposed face holds its condition
            if not on:
                R._planes(m, start[R.NORMAL[s]], s)[0][...] = c
        want = {n: a.copy(order="F") for n, a in start.items()}
        bound = R.flux_bound(m, want, conditions, schemes)
        corr = R.enforce(m, want, conditions, schemes)
        A = sum(R.face_area(m, s) for s in schemes)
        bcs = {s: ocn.OpenBoundaryCondition(c, scheme=pa if on else None) for s, (c, on) in case.items()}
        outs = []
        for _ in range(2):
            for n in "uvw":
                flds[n].set_parent(start[n])
            ocn.kernels.enforce_open_boundary_mass_conservation(grid, u, v, w, bcs)
            outs.append({n: flds[n].parent() for n in "uvw"})
        for n in "uvw":
            got = outs[0][n]
            assert np.array_equal(got, outs[1][n]), n                            # identical bits on a second call
            err = np.abs(got - want[n]).max()
            print(sorted(case), n, "max deviation", err, "bound / A", bound / A, "correction", corr)
            assert err <= bound / A, (n, err, bound / A)
        changed = {n: np.argwhere(outs[0][n] != start[n]) for n in "uvw"}
        assert sum(len(c) for c in changed.values()) == sum(int(np.prod(_face_shape(m, s))) for s in schemes)
        after = R.mass_inflow(m, outs[0], conditions, schemes)
        assert abs(after) <= 2 * bound, (after, bound)                           # the device's correction closes the restatement's budget
    # nothing is launched, nothing changes without a scheme side
    for n in "uvw":
        flds[n].set_parent(P[n])
    ocn.kernels.enforce_open_boundary_mass_conservation(grid, u, v, w, {"west": ocn.OpenBoundaryCondition(1.0)})
    assert all(np.array_equal(flds[n].parent(), P[n]) for n in "uvw")


# ---------------------------------------------------------------------------------------------------------------------
# the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA = 2e-3, {"T": 5e-3, "S": 1e-3}


def _model_pair(ocn, oracle, arch, case, timestepper):
    F, O_, PA = ocn.FieldBoundaryConditions, ocn.OpenBoundaryCondition, ocn.PerturbationAdvection
    if case == "bbb_stretched":
        size, z = (9, 20, 13), tanh_faces(13)
        closure, nu, kappa = ocn.ScalarDiffusivity(ν=NU, κ=KAPPA), NU, (KAPPA["T"], KAPPA["S"])
        pa = PA(0.3, 2.0)
        bcs = {"u": F(west=O_(0.2, scheme=pa), east=O_(0.2, scheme=pa)), "w": F(bottom=O_(0.05, scheme=pa), top=O_(0.05, scheme=pa))}
        ybcs = {"u": {"west": ("open", 0.2), "east": ("open", 0.2)}, "w": {"bottom": ("open", 0.05), "top": ("open", 0.05)}}
        schemes = {s: (0.3, 2.0) for s in ("west", "east", "bottom", "top")}
        offset = 0.2
    else:                                   # the inflow / outflow channel: imposed constant inflow, radiating outflow; FFT solver
        size, z = (12, 10, 8), (-1.0, 0.0)
        closure, nu, kappa = None, 0.0, (0.0, 0.0)
        bcs = {"u": F(west=O_(1.0), east=O_(1.0, scheme=PA(0.1, INF)))}
        ybcs = {"u": {"west": ("open", 1.0), "east": ("open", 1.0)}}
        schemes = {"east": (0.1, INF)}
        offset = 1.0
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=(ocn.Bounded,) * 3)
    g_cpu = oracle.Grid(size, topology=(1, 1, 1), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), timestepper=timestepper, closure=closure, boundary_conditions=bcs)
    yard = R.OpenBoundaryOrchestrated(oracle, g_cpu, 2, nu, kappa, closure="oracle", bcs=ybcs, schemes=schemes)
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 23)
    vals["u"] = vals["u"] + offset          # a mean flow through the open faces
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["T"], c1=vals["S"])
    return grid, model, yard, schemes


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("case", ["bbb_stretched", "channel"])
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, case, timestepper):
    """3 steps; every field and p to 1e-12 (p on the scale of test_gpu_parity.test_time_step_parity_10_steps), the clock `==`"""
    grid, model, yard, schemes = _model_pair(ocn, oracle, arch, case, timestepper)
    assert model.get_option("open_boundary_scheme_sides") == len(schemes) and model.get_option("open_boundary_launches") == 3
    core = (slice(3, -3),) * 3
    for gn, cn in zip(("u", "v", "w", "T", "S"), yard.names):                   # set!: fill, step with Δt = 0, projection
        assert rel_err(model.fields()[gn].parent()[core], yard.U[cn][core]) < 1e-12, gn
    dt = 0.05 / grid.Nx
    for _ in range(3):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    for gn, cn in zip(("u", "v", "w", "T", "S"), yard.names):
        a, b = model.fields()[gn].parent()[core], yard.U[cn][core]
        assert np.all(np.isfinite(a))
        print(case, timestepper, gn, rel_err(a, b))
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = model.pressures.pNHS.parent()[core], yard.p[core]
    pscale = max(np.abs(b).max(), umax * max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / dt)
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == 3
    assert model.clock.last_stage_Δt == yard.last_stage_dt
    # the scheme did something: the boundary values left the imposed value
    m = Metrics.of_grid(grid)
    for s in schemes:
        B = R._planes(m, model.fields()[R.NORMAL[s]].parent(), s)[0]
        assert np.abs(B - yard.bcs[R.NORMAL[s]][s][1]).max() > 1e-6, s
    assert model.get_option("graph_replays") == 0
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's tests
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_mass_conservation(ocn, arch):
    """test_open_boundary_condition_mass_conservation (test_boundary_conditions_integration.jl:164-182, 376-384): (8, 8, 8) BBB, U₀ = 1,
    PerturbationAdvection(1e-1, Inf) on west and east of u, u = 1 + 1e-2 rand, RK3, Δt = 0.1 Δz / max|u|; 20 steps, the statement holding
    after every one of them: |Σ div V| <= 5 eps, the reference's own bound"""
    F, O_, pa = ocn.FieldBoundaryConditions, ocn.OpenBoundaryCondition, ocn.PerturbationAdvection(1e-1, INF)
    grid = ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1), topology=(ocn.Bounded,) * 3)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=(), timestepper="RungeKutta3",
                                    boundary_conditions={"u": F(west=O_(1.0, scheme=pa), east=O_(1.0, scheme=pa))})
    rng = np.random.default_rng(29)
    ocn.set_model(model, u=1 + 1e-2 * rng.random(grid.interior_size(model.velocities.u.loc)))
    m = Metrics.of_grid(grid)
    dt = 0.1 * float(m.dzc[m.H[2]:m.H[2] + m.N[2]].min()) / np.abs(model.velocities.u.interior()).max()        # minimum_zspacing(grid)
    worst = 0.0
    for _ in range(20):
        ocn.time_step(model, dt)
        U = {n: f.parent() for n, f in zip("uvw", model.velocities)}
        worst = max(worst, abs(R.integrated_divergence(m, U)))
    print("max |Σ div V| over 20 steps:", worst, "bound", 5 * EPS)
    assert worst <= 5 * EPS
    assert np.abs(model.velocities.u.interior()[0] - 1.0).max() > 1e-6                   # the west face radiates: it is not the imposed 1
    model.close()


@pytest.mark.parametrize("orientation", [0, 1, 2])
def test_reference_relaxation(ocn, arch, orientation):
    """test_perturbation_advection_open_boundary_conditions, second half (:145-160): a 1-D Bounded grid of 4 cells, forcing 0.1,
    OpenBoundaryCondition(t -> 0.1 t, scheme = PerturbationAdvection(inflow_timescale = 0.01, outflow_timescale = 0.5)), AB2, 100 steps of
    0.1. The time-dependent value is the caller's to refresh: the fill evaluates it after the tick, at t + Δt."""
    from oldoceananigans_jl_amd import _lib
    topo = tuple(ocn.Bounded if d == orientation else ocn.Flat for d in range(3))
    grid = ocn.RectilinearGrid(arch, size=(4,), topology=topo, **{"xyz"[orientation]: (0.0, 4.0)})
    name = "uvw"[orientation]
    pa = ocn.PerturbationAdvection(inflow_timescale=0.01, outflow_timescale=0.5)
    lo, hi = R.SIDES[2 * orientation], R.SIDES[2 * orientation + 1]
    forcing = np.full(tuple(grid.size), 0.1)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=(), timestepper="QuasiAdamsBashforth2", forcing={name: ocn.Forcing(forcing)},
                                    boundary_conditions={name: ocn.FieldBoundaryConditions(**{lo: ocn.OpenBoundaryCondition(0.0, scheme=pa),
                                                                                             hi: ocn.OpenBoundaryCondition(0.0, scheme=pa)})})
    for step in range(100):
        t = model.clock.time + 0.1
        for side in (2 * orientation, 2 * orientation + 1):
            _lib.check(_lib.lib().ocn_model_set_boundary_condition(model.handle, name.encode(), side, 4, 0.1 * t))
        ocn.time_step(model, 0.1)
    assert model.get_option("open_boundary_scheme_sides") == 2                           # replacing the value kept the scheme
    u = model.fields()[name].interior()
    print("orientation", orientation, "u =", u.ravel())
    assert u.size == 5 and np.all(np.abs(u - 1.0) <= 0.1)
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# unchanged behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_imposed_open_conditions_are_what_they_were(ocn, arch):
    """a model with imposed open conditions only: the same bits as with enabled = 0 set explicitly on every open side, no scheme side and
    no added launch reported; a scheme on the same model then changes the result"""
    from oldoceananigans_jl_amd import _lib
    F, O_ = ocn.FieldBoundaryConditions, ocn.OpenBoundaryCondition
    grid = ocn.RectilinearGrid(arch, size=(12, 10, 8), extent=(1, 1, 1), topology=(ocn.Bounded, ocn.Periodic, ocn.Bounded))
    rng = np.random.default_rng(31)
    arr = np.asfortranarray(1.0 + 0.01 * rng.standard_normal((10, 8)))
    arr += 1.0 - arr.mean()                                                              # balanced by hand: the imposed form needs it

    def run(explicit_off, scheme):
        bcs = {"u": F(west=O_(1.0), east=O_(arr, scheme=ocn.PerturbationAdvection(0.1, INF) if scheme else None))}
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), boundary_conditions=bcs)
        if explicit_off:
            for side in (0, 1):
                _lib.check(_lib.lib().ocn_model_set_open_boundary_scheme(model.handle, b"u", side, 0, 0.0, INF))
        vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 37)
        vals["u"] = vals["u"] + 1.0
        ocn.set_model(model, **vals)
        for _ in range(3):
            ocn.time_step(model, 0.002)
        out = {n: f.parent() for n, f in model.fields().items()}
        out["p"] = model.pressures.pNHS.parent()
        report = (model.get_option("open_boundary_scheme_sides"), model.get_option("open_boundary_launches"))
        model.close()
        return out, report

    base, report = run(False, False)
    assert report == (0, 0)
    off, report_off = run(True, False)
    assert report_off == (0, 0)
    for n in base:
        assert np.array_equal(base[n], off[n]), n
    east = base["u"][3 + 12, 3:-3, 3:-3]
    assert np.array_equal(east, arr)                                                     # the imposed face holds its condition
    radiating, report_on = run(False, True)
    assert report_on == (1, 3)
    assert not np.array_equal(radiating["u"], base["u"])
