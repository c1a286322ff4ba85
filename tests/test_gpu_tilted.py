"""Tilted domains on the MI355X -- buoyancy = BuoyancyForce(formulation; gravity_unit_vector) and coriolis = ConstantCartesianCoriolis --
against the numpy restatement (tests/tilted_reference.py, pinned on the CPU by tests/test_tilted_host.py):
  * the raw kernels == the restatement (np.array_equal): ocn_add_cartesian_coriolis, ocn_add_buoyancy_acceleration (both buoyancy kinds),
    ocn_update_hydrostatic_pressure_tilted (with ĝ_z = 1 == ocn_update_hydrostatic_pressure), a launch range, the exact f × U of uniform fields;
  * the model (RK3 and AB2) against the orchestrated yardstick, 1e-12, on the three grids; the unfused paths == the default one; a
    gravity_unit_vector of (0, 0, -1) == the bare formulation;
  * the reference's own tests: stratified_fluid_remains_at_rest_with_tilted_gravity_{buoyancy,temperature}_tracer (test_dynamics.jl:263-355)
    and inertial_oscillations_work_with_rotation_in_different_axis (:357-397)."""
import math

import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import tilted_reference as T
import vertically_implicit_reference as R

pytestmark = pytest.mark.gpu

SQRT_EPS = math.sqrt(R.EPS)
# (Periodic, Periodic, Bounded) 8 x 6 x 10 tanh-stretched; (Periodic, Flat, Bounded) 8 x 8; (Bounded, Bounded, Bounded) 12 x 10 x 8: every
# interpolation with and without its Flat identity, the wall-face exclusion of each velocity, sizes that are no multiple of the 64 x 4 block
CASES = {
    "ppb_stretched": dict(size=(8, 6, 10), topo=("Periodic", "Periodic", "Bounded"), stretched=True),
    "pfb": dict(size=(8, 8), topo=("Periodic", "Flat", "Bounded"), stretched=False),
    "bbb": dict(size=(12, 10, 8), topo=("Bounded", "Bounded", "Bounded"), stretched=False),
}
TRIMMED = (2, 7, 2, 5, 3, 9)                              # a launch range on ppb_stretched
GRAV, ALPHA, BETA = 9.80665, 1.67e-4, 7.8e-4


def _grids(ocn, oracle, arch, name):
    """the same grid for the library and, when `oracle` is given, for the oracle"""
    c = CASES[name]
    topo = c["topo"]
    Nz = c["size"][-1]
    z = tanh_faces(Nz) if c["stretched"] else (-1.0, 0.0)
    kw = {d: (0.0, 1.0) for d, t in zip("xy", topo) if t != "Flat"}
    grid = ocn.RectilinearGrid(arch, size=c["size"], topology=tuple(getattr(ocn, t) for t in topo), z=z, **kw)
    g_cpu = None
    if oracle is not None:
        full = tuple(grid.size)
        g_cpu = oracle.Grid(full, topology=tuple({"Periodic": 0, "Bounded": 1, "Flat": 3}[t] for t in topo), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    return grid, g_cpu


def _smooth_fields(ocn, grid, seed, names):
    """O(1) smooth values plus a little noise over the WHOLE parent array (the halos hold the continuation: filled) ->
    (dict name -> Field, dict name -> parent array); names of u, v, w, c (a tracer), S (a salinity-like tracer), G* (tendencies)"""
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds, parents = {}, {}
    for q, n in enumerate(names):
        f = make.get(n[-1], ocn.CenterField)(grid)
        I, J, K = np.ogrid[:f.shape[0], :f.shape[1], :f.shape[2]]
        a = 0.6 * np.sin(0.7 * I + seed + q) * np.cos(0.5 * J + 0.2 * q) + 0.4 * np.cos(0.9 * K + 0.3 * I) + 0.05 * rng.standard_normal(f.shape)
        if n == "S":
            a = a + 35.0
        a = np.asfortranarray(a)
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


class _Tracer:
    """BuoyancyTracer / SeawaterBuoyancy with the constants of this file"""

    @staticmethod
    def of(ocn, kind):
        if kind == 1:
            return ocn.BuoyancyTracer()
        return ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(ALPHA, BETA), GRAV)


# ---------------------------------------------------------------------------------------------------------------------
# raw kernels == restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cartesian_coriolis_is_the_restatement(ocn, arch, name):
    """all three components of f nonzero: G_u, G_v, G_w == G - f × U over each velocity's cells (wall faces excluded), the rest of the
    parent arrays keeping their bits; on ppb_stretched once more over a launch range"""
    grid, _ = _grids(ocn, None, arch, name)
    m = R.Metrics.of_grid(grid)
    cor = ocn.ConstantCartesianCoriolis(fx=0.3, fy=-1.1, fz=0.7)
    f = (cor.fx, cor.fy, cor.fz)
    U, P = _smooth_fields(ocn, grid, 3, "uvw")
    for rng in [None] + ([TRIMMED] if name == "ppb_stretched" else []):
        G, G0 = _smooth_fields(ocn, grid, 7, ("Gu", "Gv", "Gw"))
        ocn.kernels.add_cartesian_coriolis(grid, cor, U["u"], U["v"], U["w"], G["Gu"], G["Gv"], G["Gw"], kernel_parameters=rng)
        want = T.add_cartesian_coriolis(m, f, P, {n: G0["G" + n].copy(order="F") for n in "uvw"}, rng=rng)
        for n in "uvw":
            got = G["G" + n].parent()
            assert np.array_equal(got, want[n]), (name, n, rng, np.abs(got - want[n]).max())
            changed = got != G0["G" + n]
            r = m.default_range(R.LOCS[n], True) if rng is None else rng
            inside = np.zeros(got.shape, dtype=bool)
            R._Window(m, r)(inside)[...] = True
            assert changed.any() and not changed[~inside].any(), (name, n, rng)


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_buoyancy_acceleration_is_the_restatement(ocn, arch, name, kind):
    grid, _ = _grids(ocn, None, arch, name)
    m = R.Metrics.of_grid(grid)
    gravity_unit_vector = (0.48, -0.6, -0.64)
    force = ocn.BuoyancyForce(_Tracer.of(ocn, kind), gravity_unit_vector=gravity_unit_vector)
    ghat = tuple(-c for c in gravity_unit_vector)
    C_, P = _smooth_fields(ocn, grid, 5, ("c", "S"))
    tracers = {"b": C_["c"], "T": C_["c"], "S": C_["S"]}
    b = T.buoyancy_perturbation(kind, P["c"], P["S"], GRAV, ALPHA, BETA)
    for rng in [None] + ([TRIMMED] if name == "ppb_stretched" else []):
        G, G0 = _smooth_fields(ocn, grid, 9, ("Gu", "Gv"))
        ocn.kernels.add_buoyancy_acceleration(grid, force, tracers, G["Gu"], G["Gv"], kernel_parameters=rng)
        want = T.add_buoyancy_acceleration(m, ghat, b, {n: G0["G" + n].copy(order="F") for n in "uv"}, rng=rng)
        for n in "uv":
            got = G["G" + n].parent()
            assert np.array_equal(got, want[n]), (name, kind, n, rng, np.abs(got - want[n]).max())
            # along a Flat y the y average is the identity: the term is ĝ_y b itself
            assert (got != G0["G" + n]).any()


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_tilted_hydrostatic_pressure_is_the_restatement(ocn, arch, name, kind):
    """pHY′ == the ĝ_z recurrence over i = 0:Nx+1, j = 0:Ny+1 (everything else keeps its bits); with ĝ_z = 1 == ocn_update_hydrostatic_pressure"""
    grid, _ = _grids(ocn, None, arch, name)
    m = R.Metrics.of_grid(grid)
    C_, P = _smooth_fields(ocn, grid, 11, ("c", "S"))
    tracers = {"b": C_["c"], "T": C_["c"], "S": C_["S"]}
    b = T.buoyancy_perturbation(kind, P["c"], P["S"], GRAV, ALPHA, BETA)
    formulation = _Tracer.of(ocn, kind)

    def run(fn, buoyancy):
        p = ocn.CenterField(grid)
        p.set_parent(np.full(p.shape, 7.0, order="F"))
        fn(grid, buoyancy, tracers, p)
        return p.parent()
    gz = -0.64
    got = run(ocn.kernels.update_hydrostatic_pressure_tilted, ocn.BuoyancyForce(formulation, gravity_unit_vector=(0.48, -0.6, gz)))
    want = T.hydrostatic_pressure(m, -gz, b, np.full(got.shape, 7.0, order="F"))
    assert np.array_equal(got, want), (name, kind, np.abs(got - want).max())
    assert (got != 7.0).any() and (got == 7.0).any()
    vertical = run(ocn.kernels.update_hydrostatic_pressure_tilted, ocn.BuoyancyForce(formulation, gravity_unit_vector=(0, 0, -1)))
    plain = run(ocn.kernels.update_hydrostatic_pressure, formulation)
    assert np.array_equal(vertical, plain) and np.array_equal(plain, T.hydrostatic_pressure(m, 1.0, b, np.full(got.shape, 7.0, order="F")))


def test_uniform_fields_give_the_exact_cross_product_on_the_device(ocn, arch):
    """U = (2, -0.5, 4), f = (0.25, -2, 1.5) on a triply periodic 6 x 5 x 4 grid: every product is exact, G == -(f × U) at every point;
    b ≡ 1: G_u == -gravity_unit_vector[0], G_v == -gravity_unit_vector[1] (tests/test_tilted_host.py holds the restatement to the same)"""
    grid = ocn.RectilinearGrid(arch, size=(6, 5, 4), extent=(1, 1, 1))
    Uv, f = (2.0, -0.5, 4.0), (0.25, -2.0, 1.5)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    U, G = {}, {}
    for n, val in zip("uvw", Uv):
        U[n], G[n] = make[n](grid), make[n](grid)
        U[n].set_parent(np.full(U[n].shape, val, order="F"))
        G[n].set_parent(np.zeros(G[n].shape, order="F"))
    ocn.kernels.add_cartesian_coriolis(grid, ocn.ConstantCartesianCoriolis(fx=f[0], fy=f[1], fz=f[2]), U["u"], U["v"], U["w"], G["u"], G["v"], G["w"])
    cross = (f[1] * Uv[2] - f[2] * Uv[1], f[2] * Uv[0] - f[0] * Uv[2], f[0] * Uv[1] - f[1] * Uv[0])
    assert cross == (-7.25, 2.0, 3.875)
    for n, want in zip("uvw", cross):
        assert np.all(G[n].interior() == -want), (n, want)
    b = ocn.CenterField(grid)
    b.set_parent(np.ones(b.shape, order="F"))
    for n in "uv":
        G[n].set_parent(np.zeros(G[n].shape, order="F"))
    gravity_unit_vector = (0.6, 0.8, 0.0)
    ocn.kernels.add_buoyancy_acceleration(grid, ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=gravity_unit_vector), {"b": b}, G["u"], G["v"])
    assert np.all(G["u"].interior() == -gravity_unit_vector[0]) and np.all(G["v"].interior() == -gravity_unit_vector[1])


# ---------------------------------------------------------------------------------------------------------------------
# the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA = 2e-3, 5e-3
THETA = 0.3
MODEL_CASES = {
    # case: grid, timestepper, steps, closure, gravity_unit_vector, rotation vector, backgrounds
    "A": ("ppb_stretched", "RungeKutta3", 3, True, (0.48, -0.6, -0.64), (0.3, -1.1, 0.7), False),
    "B": ("ppb_stretched", "QuasiAdamsBashforth2", 2, True, (0.48, -0.6, -0.64), (0.3, -1.1, 0.7), False),
    # the tilted bottom boundary layer: ẑ = (sin θ, 0, cos θ) is both the rotation axis and minus the gravity vector; backgrounds v and b
    "C": ("pfb", "RungeKutta3", 3, True, (-math.sin(THETA), 0.0, -math.cos(THETA)), (0.9 * math.sin(THETA), 0.0, 0.9 * math.cos(THETA)), True),
    "D": ("bbb", "RungeKutta3", 3, False, (0.48, -0.6, -0.64), (0.3, -1.1, 0.7), False),
}


def _model_pair(ocn, oracle, arch, case, options=None, yardstick=True):
    name, timestepper, steps, closure, gvec, fvec, backgrounds = MODEL_CASES[case]
    grid, g_cpu = _grids(ocn, oracle if yardstick else None, arch, name)
    F = ocn.FieldBoundaryConditions
    bcs = {"b": F(top=ocn.ValueBoundaryCondition(0.4), bottom=ocn.GradientBoundaryCondition(0.2))} if closure else None
    bg = None
    if backgrounds:
        bg = {"v": lambda x, y, z: 0.2 * np.tanh(4 * (z + 0.5)) + 0 * x + 0 * y,
              "b": lambda x, y, z: 0.8 * (x * math.sin(THETA) + z * math.cos(THETA)) + 0 * y}
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), timestepper=timestepper,
                                    buoyancy=ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=gvec),
                                    coriolis=ocn.ConstantCartesianCoriolis(fx=fvec[0], fy=fvec[1], fz=fvec[2]),
                                    closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA) if closure else None, boundary_conditions=bcs, background_fields=bg)
    for k, v in (options or {}).items():
        model.set_option(k, v)
    nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
    vals = smooth_state({("T" if n == "b" else n): v for n, v in nodes.items()}, 17)
    vals["b"] = vals.pop("T")
    ocn.set_model(model, **vals)
    yard = None
    if yardstick:
        background = None
        if backgrounds:
            bgf = model.background_fields
            background = {"v": bgf.velocities.v.parent(), "c0": bgf.tracers.b.parent()}
        yard = T.TiltedOrchestrated(oracle, g_cpu, 1, NU if closure else 0.0, (KAPPA if closure else 0.0,), cartesian=fvec, gravity_unit_vector=gvec,
                                    background=background, buoyancy_index=0, closure="numpy",
                                    bcs={"c0": {"top": ("value", 0.4), "bottom": ("gradient", 0.2)}} if closure else None)
        yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["b"])
    return grid, model, yard, (timestepper, steps)


def _step(ocn, model, yard, timestepper, steps, dt):
    for _ in range(steps):
        ocn.time_step(model, dt)
        if yard is not None:
            yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, case):
    """A: three RK3 steps on the stretched 8 x 6 x 10 grid, BuoyancyTracer, ĝ and f with all three components nonzero, ScalarDiffusivity,
    Value / Gradient conditions on b. B: the same, two AB2 steps. C: (Periodic, Flat, Bounded) with the tilted-slope set-up and background v
    and b. D: (Bounded, Bounded, Bounded), no closure. u, v, w, b and p to 1e-12 (the scale of p as in test_gpu_background.py), the clock =="""
    grid, model, yard, (timestepper, steps) = _model_pair(ocn, oracle, arch, case)
    assert model.get_option("coriolis_kind") == 2 and model.get_option("tilted_gravity") == 1 and model.get_option("epilogue_march_active") == 0
    dt = 0.05 / grid.Nx
    _step(ocn, model, yard, timestepper, steps, dt)
    core = tuple(slice(h, -h) if h else slice(None) for h in grid.halo_size)
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    for gn, cn in zip(("u", "v", "w", "b"), yard.names):
        a, b = model.fields()[gn].parent()[core], yard.U[cn][core]
        assert np.all(np.isfinite(a))
        print(f"case {case} {gn}: rel_err {rel_err(a, b):.3e}")
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = model.pressures.pNHS.parent()[core], yard.p[core]
    pscale = max(np.abs(b).max(), umax * max(d for d, t in zip((grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ), grid.topology) if t is not ocn.Flat) / dt)
    print(f"case {case} p: max abs difference {np.max(np.abs(a - b)):.3e} on the scale {pscale:.3e}")
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == steps
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    model.close()


@pytest.mark.parametrize("option", ["fused_epilogue", "fuse_substep"])
def test_unfused_paths_equal_the_default(ocn, arch, option):
    """case A with the stand-alone kernels (fused_epilogue = 0: buoyancy acceleration, Coriolis, hydrostatic gradient, closure in the
    reference's order) and without the substep riding in the epilogue (fuse_substep = 0): the same bits as the default path"""
    grid, default, _, (timestepper, steps) = _model_pair(ocn, None, arch, "A", yardstick=False)
    _, other, _, _ = _model_pair(ocn, None, arch, "A", options={option: 0}, yardstick=False)
    assert default.get_option(option) == 1 and other.get_option(option) == 0
    assert default.get_option("fuse_substep_active") == 1 and other.get_option("fuse_substep_active") == 0
    dt = 0.05 / grid.Nx
    _step(ocn, default, None, timestepper, steps, dt)
    _step(ocn, other, None, timestepper, steps, dt)
    for n in default.fields():
        a, b = other.fields()[n].parent(), default.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (option, n, np.abs(a - b).max())
    assert np.array_equal(other.pressures.pNHS.parent(), default.pressures.pNHS.parent())
    assert np.array_equal(other.pressures.pHY.parent(), default.pressures.pHY.parent())
    default.close()
    other.close()


def test_vertical_gravity_vector_changes_nothing(ocn, arch):
    """BuoyancyForce(BuoyancyTracer(), gravity_unit_vector = (0, 0, -1)) -- the tilted terms evaluated with ĝ = (-0, -0, 1), the per-value
    epilogue -- and the bare BuoyancyTracer() -- the marching epilogue -- after three RK3 steps: np.array_equal"""
    models = []
    for buoyancy in (ocn.BuoyancyTracer(), ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0, 0, -1))):
        grid, _ = _grids(ocn, None, arch, "ppb_stretched")
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), buoyancy=buoyancy, coriolis=ocn.FPlane(f=0.7), closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA))
        nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
        vals = smooth_state({("T" if n == "b" else n): v for n, v in nodes.items()}, 17)
        vals["b"] = vals.pop("T")
        ocn.set_model(model, **vals)
        for _ in range(3):
            ocn.time_step(model, 0.05 / grid.Nx)
        models.append(model)
    bare, vertical = models
    assert bare.get_option("tilted_gravity") == 0 and vertical.get_option("tilted_gravity") == 1
    assert bare.get_option("coriolis_kind") == vertical.get_option("coriolis_kind") == 1
    assert bare.get_option("epilogue_march_active") == 1 and vertical.get_option("epilogue_march_active") == 0
    for n in bare.fields():
        a, b = vertical.fields()[n].parent(), bare.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (n, np.abs(a - b).max())
    assert np.array_equal(vertical.pressures.pNHS.parent(), bare.pressures.pNHS.parent())
    assert np.array_equal(vertical.pressures.pHY.parent(), bare.pressures.pHY.parent())
    for m in models:
        m.close()


def test_setters_replace_one_another_and_validate(ocn, arch):
    """the model has one Coriolis; a gravity vector that is no unit vector is OCN_EINVAL; enabled = 0 is NegativeZDirection()"""
    from oldoceananigans_jl_amd import _lib
    grid, _ = _grids(ocn, None, arch, "ppb_stretched")
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=0.7))
    L = _lib.lib()
    assert model.get_option("coriolis_kind") == 1 and model.get_option("tilted_gravity") == 0
    assert L.ocn_model_set_cartesian_coriolis(model.handle, 1, 0.1, 0.2, 0.3) == 0 and model.get_option("coriolis_kind") == 2
    assert L.ocn_model_set_coriolis(model.handle, 1, 0.7) == 0 and model.get_option("coriolis_kind") == 1
    assert L.ocn_model_set_cartesian_coriolis(model.handle, 0, 0.0, 0.0, 0.0) == 0 and model.get_option("coriolis_kind") == 0
    assert L.ocn_model_set_gravity_unit_vector(model.handle, 1, 0.0, 1.0, 1.0) != 0 and model.get_option("tilted_gravity") == 0
    assert L.ocn_model_set_gravity_unit_vector(model.handle, 1, float("nan"), 0.0, 1.0) != 0
    assert L.ocn_model_set_gravity_unit_vector(model.handle, 1, 0.0, 0.6, -0.8) == 0 and model.get_option("tilted_gravity") == 1
    assert L.ocn_model_set_gravity_unit_vector(model.handle, 0, 0.0, 0.0, 0.0) == 0 and model.get_option("tilted_gravity") == 0
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own tests
# ---------------------------------------------------------------------------------------------------------------------
def _gradients_stay(ocn, model, name, dy_want, dz_want, L, N):
    """∂y and ∂z of the tracer at every face of the Bounded y and z directions, the wall faces included (Field(∂y(b)) is (c, f, c): its
    wall values come from the Gradient conditions' halos): the mean and every value ≈ the set gradient (rtol = √eps)"""
    fld = model.fields()[name]
    p = fld.parent()
    H = model.grid.halo_size
    d = L / N
    core = p[H[0]:-H[0], H[1] - 1:H[1] + N + 1, H[2] - 1:H[2] + N + 1]
    dy = np.diff(core, axis=1)[:, :, 1:-1] / d                  # (c, f, c): Ny + 1 faces
    dz = np.diff(core, axis=2)[:, 1:-1, :] / d                  # (c, c, f): Nz + 1 faces
    assert dy.shape == (4, N + 1, N) and dz.shape == (4, N, N + 1)
    print(f"{name}: ∂y mean {dy.mean()!r} (set {dy_want!r}), max |Δ| {np.abs(dy - dy_want).max():.3e}; "
          f"∂z mean {dz.mean()!r} (set {dz_want!r}), max |Δ| {np.abs(dz - dz_want).max():.3e}")
    for got, want in ((dy, dy_want), (dz, dz_want)):
        assert abs(got.mean() - want) <= SQRT_EPS * max(abs(got.mean()), abs(want))
        assert np.all(np.abs(got - want) <= SQRT_EPS * np.maximum(np.abs(got), abs(want)))


def test_stratified_fluid_remains_at_rest_with_tilted_gravity_buoyancy_tracer(ocn, arch):
    """test_dynamics.jl:263-306 as written: θ = 60, N = 32, L = 2000, (Periodic, Bounded, Bounded), g̃ = (0, sind θ, cosd θ),
    gravity_unit_vector = -g̃, b = N² (y g̃₂ + z g̃₃) with Gradient conditions on south / north / bottom / top, closure = nothing, Δt = 10
    minutes for one hour. Four cells along x instead of one (one-cell non-Flat directions are refused), as the θ = 0 test of
    tests/test_gpu_reference_tests.py"""
    from oldoceananigans_jl_amd.buoyancy import cosd, sind
    N, L, θ, N2 = 32, 2000.0, 60, 1e-5
    grid = ocn.RectilinearGrid(arch, size=(4, N, N), extent=(L, L, L), topology=(ocn.Periodic, ocn.Bounded, ocn.Bounded))
    g = (0.0, sind(θ), cosd(θ))
    buoyancy = ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=tuple(-c for c in g))
    y_bc, z_bc = ocn.GradientBoundaryCondition(N2 * g[1]), ocn.GradientBoundaryCondition(N2 * g[2])
    model = ocn.NonhydrostaticModel(grid=grid, buoyancy=buoyancy, tracers=("b",), closure=None,
                                    boundary_conditions={"b": ocn.FieldBoundaryConditions(bottom=z_bc, top=z_bc, south=y_bc, north=y_bc)})
    assert model.get_option("tilted_gravity") == 1
    ocn.set_model(model, b=lambda x, y, z: N2 * (x * g[0] + y * g[1] + z * g[2]))
    for _ in range(6):
        ocn.time_step(model, 600.0)
    assert model.clock.time == 3600.0
    _gradients_stay(ocn, model, "b", N2 * g[1], N2 * g[2], L, N)
    model.close()


def test_stratified_fluid_remains_at_rest_with_tilted_gravity_temperature_tracer(ocn, arch):
    """test_dynamics.jl:308-355 as written: SeawaterBuoyancy(), gravity_unit_vector = g̃ = (0, sind θ, cosd θ) (not negated there), T = ∂T∂z (y g̃₂
    + z g̃₃) with ∂T∂z = N² / (g₀ α) and Gradient conditions on T; otherwise as the buoyancy-tracer arm"""
    from oldoceananigans_jl_amd.buoyancy import cosd, sind
    N, L, θ, N2 = 32, 2000.0, 60, 1e-5
    grid = ocn.RectilinearGrid(arch, size=(4, N, N), extent=(L, L, L), topology=(ocn.Periodic, ocn.Bounded, ocn.Bounded))
    g = (0.0, sind(θ), cosd(θ))
    buoyancy = ocn.BuoyancyForce(ocn.SeawaterBuoyancy(), gravity_unit_vector=g)
    α, g0 = buoyancy.formulation.equation_of_state.thermal_expansion, buoyancy.formulation.gravitational_acceleration
    dTdz = N2 / (g0 * α)
    y_bc, z_bc = ocn.GradientBoundaryCondition(dTdz * g[1]), ocn.GradientBoundaryCondition(dTdz * g[2])
    model = ocn.NonhydrostaticModel(grid=grid, buoyancy=buoyancy, tracers=("T", "S"), closure=None,
                                    boundary_conditions={"T": ocn.FieldBoundaryConditions(bottom=z_bc, top=z_bc, south=y_bc, north=y_bc)})
    assert model.get_option("tilted_gravity") == 1
    ocn.set_model(model, T=lambda x, y, z: dTdz * (x * g[0] + y * g[1] + z * g[2]))
    for _ in range(6):
        ocn.time_step(model, 600.0)
    assert model.clock.time == 3600.0
    _gradients_stay(ocn, model, "T", dTdz * g[1], dTdz * g[2], L, N)
    model.close()


def test_inertial_oscillations_work_with_rotation_in_different_axis(ocn, arch):
    """test_dynamics.jl:357-397: f = 1, Δt = 1e-3 to t = π (the last step aligned), RK3; rotation about x with v = 1 against FPlane with
    u = 1. Adaptation: a triply periodic 4 x 4 x 4 grid with uniform fields instead of the all-Flat grid (which this library does not
    build); the reference's assertions on the values at (1, 1, 1)"""
    stop_time, dt = 2 * math.pi / 1 / 2, 1e-3

    def run(coriolis, **initial):
        grid = ocn.RectilinearGrid(arch, size=(4, 4, 4), extent=(1, 1, 1))
        model = ocn.NonhydrostaticModel(grid=grid, buoyancy=None, tracers=(), closure=None, timestepper="RungeKutta3", coriolis=coriolis)
        ocn.set_model(model, **{n: (lambda x, y, z: 1.0 + 0 * (x + y + z)) for n in initial})
        t, n = 0.0, 0
        while t < stop_time:                              # Simulation: Δt = min(Δt, stop_time - time) (aligned_time_step)
            ocn.time_step(model, min(dt, stop_time - t))
            t = model.clock.time
            n += 1
        assert abs(t - stop_time) <= 4 * R.EPS and n in (3142, 3143)          # (3143: the clock landed one rounding short of π)
        out = tuple(float(model.fields()[c].interior()[0, 0, 0]) for c in "uvw")
        for c in "uvw":                                   # the fields stayed uniform
            a = model.fields()[c].interior()
            assert np.all(a == a[0, 0, 0])
        model.close()
        return out
    u_x, v_x, w_x = run(ocn.ConstantCartesianCoriolis(f=1, rotation_axis=(1, 0, 0)), v=1)
    u_z, v_z, w_z = run(ocn.FPlane(f=1), u=1)
    print(f"x rotation: (u, v, w) = {(u_x, v_x, w_x)!r}; z rotation: {(u_z, v_z, w_z)!r}")
    approx = lambda a, b: abs(a - b) <= SQRT_EPS * max(abs(a), abs(b))          # noqa: E731
    assert w_z == 0
    assert u_x == 0
    assert approx(math.sqrt(v_x ** 2 + w_x ** 2), 1)
    assert approx(math.sqrt(u_z ** 2 + v_z ** 2), 1)
    assert approx(u_z, v_x)
    assert approx(v_z, w_x)
