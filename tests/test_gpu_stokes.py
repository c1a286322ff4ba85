"""stokes_drift = UniformStokesDrift on the MI355X against the numpy restatement (tests/stokes_reference.py, pinned on the CPU by
tests/test_stokes_host.py):
  * the raw kernel == the restatement (np.array_equal) on four grids, a launch range, the exact products of uniform velocities;
  * the model (RK3 and AB2) against the orchestrated yardstick, 1e-12: the drift alone, with FPlane + BuoyancyTracer + ScalarDiffusivity (the
    Langmuir set with what the yardstick has), with an array forcing on u (the term order), with a background tracer;
  * the stand-alone pass (fused_epilogue = 0) == the per-value epilogue; setting and clearing the drift on a live model;
  * an all-zero drift == no drift;
  * the reference's own tests: time_stepping_works_with_stokes_drift (test_time_stepping.jl:60-66,269-304,359-363) and the array / nothing /
    function mix (:404-413);
  * the refusals of ocn_model_set_stokes_drift."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import order_one_stokes_drift, rel_err, smooth_state, tanh_faces
import stokes_reference as S
import vertically_implicit_reference as R

pytestmark = pytest.mark.gpu

# the three grids of tests/test_gpu_tilted.py -- every average with and without its Flat identity, the wall-face exclusion of each velocity,
# sizes that are no multiple of the 64 x 4 block, a stretched z -- and a Periodic z, where k ± 1 wraps through the halo and w covers k = 1..Nz
CASES = {
    "ppb_stretched": dict(size=(8, 6, 10), topo=("Periodic", "Periodic", "Bounded"), stretched=True),
    "pfb": dict(size=(8, 8), topo=("Periodic", "Flat", "Bounded"), stretched=False),
    "bbb": dict(size=(12, 10, 8), topo=("Bounded", "Bounded", "Bounded"), stretched=False),
    "ppp": dict(size=(8, 8, 8), topo=("Periodic", "Periodic", "Periodic"), stretched=False),
}
TRIMMED = (2, 7, 2, 5, 3, 9)                              # a launch range on ppb_stretched


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
        g_cpu = oracle.Grid(tuple(grid.size), topology=tuple({"Periodic": 0, "Bounded": 1, "Flat": 3}[t] for t in topo), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    return grid, g_cpu


def _smooth_fields(ocn, grid, seed, names):
    """O(1) smooth values plus a little noise over the WHOLE parent array (the halos hold the continuation: filled) ->
    (dict name -> Field, dict name -> parent array); the last letter of a name is its velocity component"""
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds, parents = {}, {}
    for q, n in enumerate(names):
        f = make[n[-1]](grid)
        I, J, K = np.ogrid[:f.shape[0], :f.shape[1], :f.shape[2]]
        a = 0.6 * np.sin(0.7 * I + seed + q) * np.cos(0.5 * J + 0.2 * q) + 0.4 * np.cos(0.9 * K + 0.3 * I) + 0.05 * rng.standard_normal(f.shape)
        a = np.asfortranarray(a)
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


# ---------------------------------------------------------------------------------------------------------------------
# 1. the raw kernel == the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_raw_kernel_is_the_restatement(ocn, arch, name):
    """G_u, G_v, G_w == the restatement over each velocity's cells (wall faces excluded; w over k = 2..Nz on a Bounded z, 1..Nz on the
    Periodic one), the rest of the parent arrays keeping their bits; on ppb_stretched once more over a launch range"""
    grid, _ = _grids(ocn, None, arch, name)
    m = R.Metrics.of_grid(grid)
    drift = order_one_stokes_drift(ocn)
    tables = drift.tables(grid)
    U, P = _smooth_fields(ocn, grid, 3, "uvw")
    for rng in [None] + ([TRIMMED] if name == "ppb_stretched" else []):
        G, G0 = _smooth_fields(ocn, grid, 7, ("Gu", "Gv", "Gw"))
        ocn.kernels.add_stokes_drift(grid, drift, U["u"], U["v"], U["w"], G["Gu"], G["Gv"], G["Gw"], kernel_parameters=rng)
        want = S.add_stokes_drift(m, tables, P, {n: G0["G" + n].copy(order="F") for n in "uvw"}, rng=rng)
        for n in "uvw":
            got = G["G" + n].parent()
            assert np.array_equal(got, want[n]), (name, n, rng, np.abs(got - want[n]).max())
            changed = got != G0["G" + n]
            r = m.default_range(R.LOCS[n], True) if rng is None else rng
            inside = np.zeros(got.shape, dtype=bool)
            R._Window(m, r)(inside)[...] = True
            assert changed.any() and not changed[~inside].any(), (name, n, rng)
        if rng is None:
            assert m.default_range(R.LOCS["w"], True)[4] == (1 if name == "ppp" else 2)


def test_uniform_velocities_give_exact_products_on_the_device(ocn, arch):
    """w ≡ W on the stretched grid: G_u == W * ∂z_uˢ(z_c[k]) and G_v == W * ∂z_vˢ(z_c[k]) exactly (G = 0, no ∂t); u ≡ U₀, v ≡ V₀, w ≡ 0: G_w ==
    (-U₀) * ∂z_uˢ(z_f[k]) - V₀ * ∂z_vˢ(z_f[k]) with one rounding per operation and G_u, G_v == the ∂t tables (tests/test_stokes_host.py holds
    the restatement to the same)"""
    grid, _ = _grids(ocn, None, arch, "ppb_stretched")
    m = R.Metrics.of_grid(grid)
    full = order_one_stokes_drift(ocn)
    dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c = full.tables(grid)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}

    def run(drift, values):
        U, G = {}, {}
        for n in "uvw":
            U[n], G[n] = make[n](grid), make[n](grid)
            U[n].set_parent(np.full(U[n].shape, values[n], order="F"))
            G[n].set_parent(np.zeros(G[n].shape, order="F"))
        ocn.kernels.add_stokes_drift(grid, drift, U["u"], U["v"], U["w"], G["u"], G["v"], G["w"])
        return {n: R._Window(m, m.default_range(R.LOCS[n], True))(G[n].parent()) for n in "uvw"}
    W, U0, V0 = 1.7, -0.9, 2.3
    shear_only = ocn.UniformStokesDrift(dz_us=full.dz_us, dz_vs=full.dz_vs)
    G = run(shear_only, dict(u=0.0, v=0.0, w=W))
    assert np.all(G["u"] == (W * dzu_c)[None, None, :]) and np.all(G["v"] == (W * dzv_c)[None, None, :]) and not G["w"].any()
    G = run(full, dict(u=U0, v=V0, w=0.0))
    assert np.all(G["w"] == ((-U0) * dzu_f - V0 * dzv_f)[None, None, 1:grid.Nz])
    assert np.all(G["u"] == dtu_c[None, None, :]) and np.all(G["v"] == dtv_c[None, None, :])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA, FCOR = 2e-3, 5e-3, 0.7
MODEL_CASES = {
    # case: grid, timestepper, the Langmuir set (FPlane + BuoyancyTracer + ScalarDiffusivity), an array forcing on u, a background tracer
    "drift_rk3": ("ppb_stretched", "RungeKutta3", False, False, False),
    "drift_ab2": ("ppb_stretched", "QuasiAdamsBashforth2", False, False, False),
    "drift_pfb": ("pfb", "RungeKutta3", False, False, False),
    "drift_bbb": ("bbb", "RungeKutta3", False, False, False),
    "drift_ppp": ("ppp", "RungeKutta3", False, False, False),
    "langmuir_rk3": ("ppb_stretched", "RungeKutta3", True, False, False),
    "langmuir_ab2": ("ppb_stretched", "QuasiAdamsBashforth2", True, False, False),
    "forced_rk3": ("ppb_stretched", "RungeKutta3", True, True, False),
    "forced_ab2": ("ppb_stretched", "QuasiAdamsBashforth2", True, True, False),
    "background_rk3": ("ppb_stretched", "RungeKutta3", True, False, True),
    "background_ab2": ("ppb_stretched", "QuasiAdamsBashforth2", True, False, True),
}
STEPS = 3


def _model_pair(ocn, oracle, arch, case, options=None, yardstick=True, drift="default", closure=None):
    name, timestepper, langmuir, forced, background = MODEL_CASES[case]
    grid, g_cpu = _grids(ocn, oracle if yardstick else None, arch, name)
    drift = order_one_stokes_drift(ocn) if drift == "default" else drift
    forcing = 0.3 * np.random.default_rng(4).standard_normal(grid.interior_size((ocn.Face, ocn.Center, ocn.Center))) if forced else None
    bg = {"b": lambda x, y, z: 0.8 * z + 0 * x + 0 * y} if background else None
    if closure is None and langmuir:
        closure = ocn.ScalarDiffusivity(ν=NU, κ=KAPPA)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer() if langmuir else None,
                                    coriolis=ocn.FPlane(f=FCOR) if langmuir else None, closure=closure,
                                    forcing={"u": forcing} if forced else None, background_fields=bg, stokes_drift=drift)
    for k, v in (options or {}).items():
        model.set_option(k, v)
    nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
    vals = smooth_state({("T" if n == "b" else n): v for n, v in nodes.items()}, 17)
    vals["b"] = vals.pop("T")
    ocn.set_model(model, **vals)
    yard = None
    if yardstick:
        yard = S.StokesOrchestrated(oracle, g_cpu, 1, NU if langmuir else 0.0, (KAPPA if langmuir else 0.0,), stokes_tables=drift.tables(grid),
                                    background={"c0": model.background_fields.tracers.b.parent()} if background else None,
                                    buoyancy_index=0 if langmuir else None, fcor=FCOR if langmuir else None,
                                    forcing={"u": forcing} if forced else None, closure="numpy")
        yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["b"])
    return grid, model, yard, timestepper


def _step(ocn, model, yard, timestepper, steps, dt):
    for _ in range(steps):
        ocn.time_step(model, dt)
        if yard is not None:
            yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, case):
    """three steps, RK3 and AB2, on the stretched 8 x 6 x 10 grid: the drift alone; with FPlane, BuoyancyTracer and ScalarDiffusivity; that set
    with an array forcing on u (the Stokes terms come before it, and the substep then does not ride along); that set with a background
    tracer. The drift alone also on the other three grids. u, v, w, b and p to 1e-12 (the scale of p as in test_gpu_tilted.py), the clock
    ==. The drift is inside the per-value epilogue: stokes_path 2."""
    grid, model, yard, timestepper = _model_pair(ocn, oracle, arch, case)
    forced = MODEL_CASES[case][3]
    assert model.get_option("stokes_drift") == 1 and model.get_option("stokes_path") == 2 and model.get_option("epilogue_march_active") == 0
    assert model.get_option("forcing_path") == (3 if forced else 0) and model.get_option("fuse_substep_active") == (0 if forced else 1)
    dt = 0.05 / grid.Nx
    _step(ocn, model, yard, timestepper, STEPS, dt)
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
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == STEPS
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    model.close()


def test_the_drift_matters(ocn, arch):
    """the same model with and without the drift after three steps: u differs by far more than the tolerance of the comparisons above"""
    grid, with_drift, _, timestepper = _model_pair(ocn, None, arch, "langmuir_rk3", yardstick=False)
    _, without, _, _ = _model_pair(ocn, None, arch, "langmuir_rk3", yardstick=False, drift=None)
    assert without.get_option("stokes_drift") == 0 and without.get_option("stokes_path") == 0
    for model in (with_drift, without):
        _step(ocn, model, None, timestepper, STEPS, 0.05 / grid.Nx)
    for n in "uvw":
        a, b = with_drift.fields()[n].parent(), without.fields()[n].parent()
        print(f"{n}: relative difference made by the drift {rel_err(a, b):.3e}")
        assert rel_err(a, b) > 1e-6
    with_drift.close()
    without.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. path equivalence
# ---------------------------------------------------------------------------------------------------------------------
def _same(a_model, b_model, what):
    for n in a_model.fields():
        for label, get in (("field", lambda m: m.fields()[n]), ("Gn", lambda m: m.tendency(n)), ("Gm", lambda m: m.tendency(n, previous=True))):
            a, b = get(a_model).parent(), get(b_model).parent()
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (what, label, n, np.abs(a - b).max())
    assert np.array_equal(a_model.pressures.pNHS.parent(), b_model.pressures.pNHS.parent()), what


@pytest.mark.parametrize("case", ["langmuir_rk3", "langmuir_ab2", "drift_bbb"])
def test_stand_alone_pass_equals_the_epilogue(ocn, arch, case):
    """fused_epilogue 1 (the Stokes terms inside the per-value epilogue, stokes_path 2) against 0 (stokes_drift_kernel after the stand-alone
    physics kernels, stokes_path 1): fields, Gⁿ, G⁻ and pressure == after two steps"""
    grid, default, _, timestepper = _model_pair(ocn, None, arch, case, yardstick=False)
    _, other, _, _ = _model_pair(ocn, None, arch, case, options={"fused_epilogue": 0}, yardstick=False)
    assert default.get_option("stokes_path") == 2 and other.get_option("stokes_path") == 1
    assert default.get_option("fuse_substep_active") == 1 and other.get_option("fuse_substep_active") == 0
    for model in (default, other):
        _step(ocn, model, None, timestepper, 2, 0.05 / grid.Nx)
    _same(other, default, case)
    default.close()
    other.close()


def test_setting_and_clearing_the_drift_on_a_live_model(ocn, arch):
    """an AnisotropicMinimumDissipation model takes the marching epilogue; with a drift the per-value one (epilogue_march_active 0); after
    ocn_model_set_stokes_drift(model, 0, ...) the marching one again, and one step from there == a model that never had a drift"""
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    amd = lambda: ocn.AnisotropicMinimumDissipation()      # noqa: E731
    grid, model, _, _ = _model_pair(ocn, None, arch, "langmuir_rk3", yardstick=False, closure=amd())
    _, never, _, _ = _model_pair(ocn, None, arch, "langmuir_rk3", yardstick=False, closure=amd(), drift=None)
    assert model.get_option("stokes_drift") == 1 and model.get_option("epilogue_march_active") == 0 and model.get_option("stokes_path") == 2
    assert never.get_option("stokes_drift") == 0 and never.get_option("epilogue_march_active") == 1
    assert L.ocn_model_set_stokes_drift(model.handle, 0, None, None, None, None, None, None) == 0
    assert model.get_option("stokes_drift") == 0 and model.get_option("stokes_path") == 0 and model.get_option("epilogue_march_active") == 1
    dt = 0.05 / grid.Nx
    for m in (model, never):
        ocn.time_step(m, dt)
    for n in never.fields():
        a, b = model.fields()[n].parent(), never.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (n, np.abs(a - b).max())
    # set between steps: a second call replaces the first whole -- the full drift, then ∂t_uˢ alone == a model that only ever got ∂t_uˢ
    dp = C.POINTER(C.c_double)
    tables = order_one_stokes_drift(ocn).tables(grid)
    _, only, _, _ = _model_pair(ocn, None, arch, "langmuir_rk3", yardstick=False, closure=amd(), drift=None)
    ocn.time_step(only, dt)
    assert L.ocn_model_set_stokes_drift(model.handle, 1, *[t.ctypes.data_as(dp) for t in tables]) == 0
    assert model.get_option("stokes_drift") == 1 and model.get_option("epilogue_march_active") == 0
    for m in (model, only):
        assert L.ocn_model_set_stokes_drift(m.handle, 1, None, None, None, None, tables[4].ctypes.data_as(dp), None) == 0
    for m in (model, only, never):
        ocn.time_step(m, dt)
    for n in never.fields():
        a, b = model.fields()[n].parent(), only.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (n, np.abs(a - b).max())
    assert np.abs(model.fields()["u"].parent() - never.fields()["u"].parent()).max() > 1e-6
    for m in (model, only, never):
        m.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. an all-zero drift
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["langmuir_rk3", "drift_ppp"])
def test_zero_drift_changes_nothing(ocn, arch, case):
    """UniformStokesDrift() -- four zerofunctions, whose products and sums are still formed, in the per-value epilogue -- against
    stokes_drift = nothing after two steps: np.array_equal"""
    grid, zero, _, timestepper = _model_pair(ocn, None, arch, case, yardstick=False, drift=ocn.UniformStokesDrift())
    _, none, _, _ = _model_pair(ocn, None, arch, case, yardstick=False, drift=None)
    assert zero.get_option("stokes_drift") == 1 and none.get_option("stokes_drift") == 0
    for model in (zero, none):
        _step(ocn, model, None, timestepper, 2, 0.05 / grid.Nx)
    for n in none.fields():
        a, b = zero.fields()[n].parent(), none.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (n, np.abs(a - b).max())
    assert np.array_equal(zero.pressures.pNHS.parent(), none.pressures.pNHS.parent())
    zero.close()
    none.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the reference's own tests
# ---------------------------------------------------------------------------------------------------------------------
def _reference_grid(ocn, arch):
    return ocn.RectilinearGrid(arch, size=(3, 3, 3), halo=(3, 3, 3), extent=(1, 2, 3))


@pytest.mark.parametrize("which", ["zero", "parameterized"])
def test_time_stepping_works_with_stokes_drift(ocn, arch, which):
    """test_time_stepping.jl:60-66 with the drifts of :269-304: a 3 x 3 x 3 grid, halo 3, extent (1, 2, 3), one step of Δt = 1, for
    UniformStokesDrift() and the parameterised drift with parameters = 20. Adaptations: the time factors cos t / sin t are frozen at t = 0
    (time dependence is refused: the first assertion); advection = nothing becomes the library's WENO, which gives zero on this state (the
    velocities start at zero and stay uniform in x and y); StokesDrift() is asserted refused. Beyond "no crash": w and the pressure stay 0
    and u(z) = Δt ∂t_uˢ(z_c), v likewise, to rtol 1e-14 -- three substeps of at most four roundings each is <= 12 ulp, 1e-14 is about 45."""
    grid = _reference_grid(ocn, arch)
    with pytest.raises(NotImplementedError, match="StokesDrift"):
        ocn.NonhydrostaticModel(grid=grid, tracers=(), stokes_drift=ocn.StokesDrift())
    if which == "zero":
        drift = ocn.UniformStokesDrift()
    else:
        moving = ocn.UniformStokesDrift(dt_us=lambda z, t, h: math.exp(z / h) * math.cos(t), dt_vs=lambda z, t, h: math.exp(z / h) * math.cos(t),
                                        dz_us=lambda z, t, h: math.exp(z / h) / h * math.sin(t), dz_vs=lambda z, t, h: math.exp(z / h) / h * math.sin(t),
                                        parameters=20)
        with pytest.raises(NotImplementedError, match="time dependence"):
            ocn.NonhydrostaticModel(grid=grid, tracers=(), stokes_drift=moving)
        drift = ocn.UniformStokesDrift(dt_us=lambda z, t, h: math.exp(z / h) * math.cos(0.0), dt_vs=lambda z, t, h: math.exp(z / h) * math.cos(0.0),
                                       dz_us=lambda z, t, h: math.exp(z / h) / h * math.sin(0.0), dz_vs=lambda z, t, h: math.exp(z / h) / h * math.sin(0.0),
                                       parameters=20)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=(), stokes_drift=drift)
    ocn.time_step(model, 1)
    assert model.clock.time == 1.0 and model.clock.iteration == 1
    zc = grid.nodes((ocn.Center, ocn.Center, ocn.Center))[2]
    want = np.zeros(3) if which == "zero" else np.exp(zc.ravel() / 20)
    for n in "uv":
        got = model.fields()[n].interior()
        print(f"{which} {n}: max relative deviation from Δt ∂t_Uˢ {np.max(np.abs(got - want[None, None, :]) / np.maximum(np.abs(want), 1e-300)[None, None, :]):.3e}")
        assert np.all(np.abs(got - want[None, None, :]) <= 1e-14 * np.abs(want)[None, None, :]), n
    assert not model.fields()["w"].interior().any() and not model.pressures.pNHS.interior().any()
    model.close()


def test_uniform_stokes_drift_with_array_nothing_and_function(ocn, arch):
    """test_time_stepping.jl:404-413: UniformStokesDrift(grid, ∂z_vˢ = nothing, ∂t_uˢ = (z, t) -> exp(z / 20)) -- an array default, a nothing and
    a function in one drift -- one step of Δt = 1. On 3 x 3 x 3 (extent (1, 1, 1)) because one-cell directions are refused here."""
    grid = ocn.RectilinearGrid(arch, size=(3, 3, 3), extent=(1, 1, 1))
    drift = ocn.UniformStokesDrift(grid, dz_vs=None, dt_us=lambda z, t: math.exp(z / 20))
    assert isinstance(drift.dz_us, np.ndarray) and isinstance(drift.dt_vs, np.ndarray) and callable(drift.dt_us)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=(), stokes_drift=drift)
    ocn.time_step(model, 1)
    zc = grid.nodes((ocn.Center, ocn.Center, ocn.Center))[2].ravel()
    got = model.fields()["u"].interior()
    assert np.all(np.abs(got - np.exp(zc / 20)[None, None, :]) <= 1e-14 * np.exp(zc / 20)[None, None, :])
    assert not model.fields()["v"].interior().any() and not model.fields()["w"].interior().any()
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C ABI's refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_leave_the_model_untouched(ocn, arch):
    """NULL model and a Flat z: OCN_EINVAL (-1); a partitioned handle (one rank that is its own neighbour): OCN_ENOTSUP (-2); a refused call
    leaves stokes_drift at its previous answer"""
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import distributed as dist
    L = _lib.lib()
    none = (None,) * 6
    assert L.ocn_model_set_stokes_drift(None, 1, *none) == -1 and L.ocn_last_error()
    flat = ocn.RectilinearGrid(arch, size=(8, 8), extent=(1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Flat))
    model = ocn.NonhydrostaticModel(grid=flat, tracers=())
    assert L.ocn_model_set_stokes_drift(model.handle, 1, *none) == -1 and b"z" in L.ocn_last_error()
    assert model.get_option("stokes_drift") == 0 and model.get_option("stokes_path") == 0
    model.close()
    uid = C.create_string_buffer(128)
    _lib.check(L.ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    grid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    part = dist.LibraryDistributedModel(grid=grid, tracers=())
    assert L.ocn_model_set_stokes_drift(part.handle, 1, *none) == -2 and b"partitioned" in L.ocn_last_error()
    assert part.get_option("stokes_drift") == 0
    with pytest.raises(NotImplementedError, match="partitioned"):
        dist.LibraryDistributedModel(grid=grid, tracers=(), stokes_drift=order_one_stokes_drift(ocn))
    part.close()
    ctx.close()
    # a live drift survives a refused ... there is no refusable call on a valid single-GPU model with a z direction: the raw kernel's instead
    g3, _ = _grids(ocn, None, arch, "ppb_stretched")
    U, _ = _smooth_fields(ocn, g3, 3, "uvw")
    G, G0 = _smooth_fields(ocn, g3, 7, ("Gu", "Gv", "Gw"))
    bad = (C.c_int * 6)(1, g3.Nx + 1, 1, g3.Ny, 1, g3.Nz)
    args = (g3.handle,) + none + (U["u"].data, U["v"].data, U["w"].data, G["Gu"].data, G["Gv"].data, G["Gw"].data)
    assert L.ocn_add_stokes_drift(*args, None, bad, None) == -1
    assert L.ocn_add_stokes_drift(g3.handle, *none, None, U["v"].data, U["w"].data, G["Gu"].data, G["Gv"].data, G["Gw"].data, None, None, None) == -1
    for n in "uvw":
        assert np.array_equal(G["G" + n].parent(), G0["G" + n])
