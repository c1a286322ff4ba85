"""Smagorinsky(coefficient = DynamicCoefficient(...)) on the MI355X: the coefficient kernels, the averages and the eddy viscosity bit for bit
against the numpy restatement (tests/dynamic_smagorinsky_reference.py, pinned by closed forms in tests/test_dynamic_smagorinsky_host.py),
free-standing and inside RK3 and QuasiAdamsBashforth2 models, with directional and Lagrangian averaging."""
import ctypes as C

import numpy as np
import pytest

import dynamic_smagorinsky_reference as R

pytestmark = pytest.mark.gpu

OCN_EINVAL, OCN_ENOTSUP, OCN_ESTATE = -1, -2, -3          # include/ocn_mi355x.h
DIMS = {1: 1, (1, 2): 3, (2, 3): 6, ":": 7}


def _velocities(ocn, grid, vals):
    """device fields of interior values with filled halos -> (dict name -> Field, dict name -> parent array)"""
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds = {n: make[n](grid).set(vals[n]) for n in "uvw"}
    ocn.fill_halo_regions(list(flds.values()))
    return flds, {n: f.parent() for n, f in flds.items()}


def _interior(grid, a):
    return a[grid.Hx:grid.Hx + grid.Nx, grid.Hy:grid.Hy + grid.Ny, grid.Hz:grid.Hz + grid.Nz]


def _viscosity(ocn, grid, coefficient, fields, flds):
    nu = ocn.CenterField(grid)
    ocn.kernels.compute_dynamic_smagorinsky_viscosity(grid, coefficient, fields, flds["u"], flds["v"], flds["w"], nu)
    return _interior(grid, nu.parent())


@pytest.fixture(scope="module")
def cases(ocn, arch):
    """per grid: the grid, the device velocities, their parents and the restatement's Σ, Σ̄, LM, MM -- computed once, never modified"""
    out = {}
    for name in R.GRIDS:
        grid = R.make_grid(ocn, arch, name)
        vals, _ = R.case_values(grid, "none")
        flds, Pn = _velocities(ocn, grid, vals)
        d = R.DynamicDriver(grid, 7)
        d.coefficient_update(Pn["u"], Pn["v"], Pn["w"])
        out[name] = (grid, flds, Pn, d)
    return out


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_sigma_and_lm_mm_are_the_restatement_bit_for_bit(ocn, cases, name):
    grid, flds, Pn, want = cases[name]
    dc = ocn.DynamicCoefficient(averaging=(1, 2))
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields)
    assert np.array_equal(fields["Sigma"].parent(), want.Sigma)                    # the halo stays 0
    assert np.array_equal(fields["Sigma_bar"].parent(), want.Sigma_bar)
    assert np.array_equal(_interior(grid, fields["LM"].parent()), want.LM)
    assert np.array_equal(_interior(grid, fields["MM"].parent()), want.MM)
    assert np.isfinite(want.LM).all() and want.MM.min() > 0


@pytest.mark.parametrize("dims", list(DIMS), ids=["x", "xy", "yz", "xyz"])
@pytest.mark.parametrize("name", list(R.GRIDS))
def test_directional_averages_and_viscosity_are_exact(ocn, cases, name, dims):
    """𝒥 = Average(LM | MM, dims) in the reduction's reproducible order; νₑ == viscosity(device 𝒥)"""
    grid, flds, Pn, base = cases[name]
    dc = ocn.DynamicCoefficient(averaging=dims)
    assert dc.averaging_mask == DIMS[dims]
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields)
    m = R.Metrics(grid)
    J_LM, J_MM = fields["J_LM"].parent(), fields["J_MM"].parent()
    kept = tuple(slice(0, 1) if dc.averaging_mask >> d & 1 else slice(h, h + n) for d, (h, n) in enumerate(zip(grid.halo_size, grid.size)))
    assert J_LM.shape == tuple(1 if dc.averaging_mask >> d & 1 else n + 2 * h for d, (h, n) in enumerate(zip(grid.halo_size, grid.size)))
    want_LM = R.ordered_average(grid, R._on_interior(m, base.LM), dc.averaging_mask)
    want_MM = R.ordered_average(grid, R._on_interior(m, base.MM), dc.averaging_mask)
    assert np.array_equal(J_LM[kept], want_LM) and np.array_equal(J_MM[kept], want_MM)
    nu = _viscosity(ocn, grid, dc, fields, flds)
    assert np.array_equal(nu, R.viscosity(m, Pn["u"], Pn["v"], Pn["w"], J_LM[kept], J_MM[kept], dc.minimum_numerator))
    assert np.isfinite(nu).all() and nu.max() > 0


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_minimum_numerator_clamps_part_of_the_coefficients(ocn, cases, name):
    """a minimum_numerator chosen on the CPU from the restatement's 𝒥ᴸᴹ (the case test_dynamic_smagorinsky_host.py asserts the split of)"""
    grid, flds, Pn, base = cases[name]
    m = R.Metrics(grid)
    want_LM = R.ordered_average(grid, R._on_interior(m, base.LM), 1)
    jmin = R.clamping_minimum(want_LM)
    assert 0.1 <= np.mean(want_LM < jmin) <= 0.9
    dc = ocn.DynamicCoefficient(averaging=1, minimum_numerator=jmin)
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields)
    J_LM = fields["J_LM"].parent()[:, grid.Hy:grid.Hy + grid.Ny, grid.Hz:grid.Hz + grid.Nz]
    J_MM = fields["J_MM"].parent()[:, grid.Hy:grid.Hy + grid.Ny, grid.Hz:grid.Hz + grid.Nz]
    assert np.array_equal(J_LM, want_LM)                                     # the field itself is not clamped, the coefficient is
    nu = _viscosity(ocn, grid, dc, fields, flds)
    assert np.array_equal(nu, R.viscosity(m, Pn["u"], Pn["v"], Pn["w"], J_LM, J_MM, jmin))
    unclamped = R.viscosity(m, Pn["u"], Pn["v"], Pn["w"], J_LM, J_MM, -np.inf)
    assert 0.1 <= np.mean(nu != unclamped) <= 0.9


@pytest.mark.parametrize("averaging", [(1, 2), "lagrangian"])
def test_a_slab_at_rest_has_zero_viscosity(ocn, arch, averaging):
    """velocities that vanish in the levels 3 .. 10 of 12 and are smooth elsewhere: in the slab's core MM = 0 (with (1, 2) the whole level:
    𝒥ᴹᴹ = 0 and the coefficient's quotient is discarded) and νₑ is exactly 0; νₑ is finite everywhere and equals the restatement"""
    grid = R.make_grid(ocn, arch, "ppp")
    vals, _ = R.case_values(grid, "none")
    for n in "uvw":
        vals[n] = vals[n].copy()
        vals[n][:, :, 2:10] = 0.0
    flds, Pn = _velocities(ocn, grid, vals)
    lagrangian = averaging == "lagrangian"
    dc = ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging() if lagrangian else averaging)
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    d = R.DynamicDriver(grid, dc.averaging_mask)
    ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields)
    d.coefficient_update(Pn["u"], Pn["v"], Pn["w"])
    if lagrangian:
        ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields, Δt=0.05, initialising=False)
        d.coefficient_update(Pn["u"], Pn["v"], Pn["w"], 0.05, False)
        assert np.array_equal(fields["J_MM"].parent(), d.J_MM) and np.array_equal(fields["J_LM"].parent(), d.J_LM)
    else:
        assert np.all(_interior(grid, fields["MM"].parent())[:, :, 5:7] == 0.0)
        assert np.all(fields["J_MM"].parent()[0, 0, grid.Hz + 5:grid.Hz + 7] == 0.0)
    nu = _viscosity(ocn, grid, dc, fields, flds)
    assert np.isfinite(nu).all() and nu.max() > 0
    assert np.all(nu[:, :, 5:7] == 0.0)
    assert np.array_equal(nu, d.viscosity(Pn["u"], Pn["v"], Pn["w"]))


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_lagrangian_updates_follow_the_restatement(ocn, cases, name):
    """the initialising update and three averaging updates, the restatement advanced alongside: the WHOLE parents of 𝒥ᴸᴹ, 𝒥ᴹᴹ (the halos hold
    the initial mean) and of 𝒥⁻ agree exactly, as the interpolated values of test_gpu_particles.py do. Δt is such that some displacements are
    clamped to one spacing and some are not"""
    grid, flds, Pn, _ = cases[name]
    dc = ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging(), minimum_numerator=1e-12)
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    d = R.DynamicDriver(grid, 0, minimum_numerator=1e-12)
    dt = 2.0 * grid.Δxᶜᵃᵃ / 0.5                    # |u| <= 0.51: displacements up to two spacings in x
    for n in range(4):
        ocn.kernels.dynamic_smagorinsky_update(grid, dc, flds["u"], flds["v"], flds["w"], fields, Δt=dt, initialising=n == 0)
        d.coefficient_update(Pn["u"], Pn["v"], Pn["w"], dt, n == 0)
        for key in ("J_LM", "J_MM", "J_LM_prev", "J_MM_prev"):
            assert np.array_equal(fields[key].parent(), getattr(d, key)), (n, key)
    assert len(d.clamped) == 3 and all(0.05 < c < 0.95 for c in d.clamped), d.clamped
    halo = np.ones(d.J_LM.shape, dtype=bool)
    halo[grid.Hx:-grid.Hx, grid.Hy:-grid.Hy, grid.Hz:-grid.Hz] = False
    got = fields["J_MM"].parent()
    assert np.all(got[halo] == got[0, 0, 0]) and not np.all(got[~halo] == got[0, 0, 0])
    assert fields["J_LM"].parent().min() >= 1e-12
    nu = _viscosity(ocn, grid, dc, fields, flds)
    assert np.array_equal(nu, d.viscosity(Pn["u"], Pn["v"], Pn["w"])) and np.isfinite(nu).all()


FORMS = [(1, (1, None, None)), ((1, 2), (1, 1, None)), ((2, 3), (None, 1, 1)), (":", (1, 1, 1))]


def test_field_sizes(ocn, arch):
    """the sizes test_turbulence_closures.jl:395-433 asserts, for the five averaging forms"""
    grid = ocn.RectilinearGrid(arch, size=(4, 5, 6), extent=(1, 2, 3))
    size = lambda f: f.interior().shape                                     # noqa: E731
    for averaging, reduced in FORMS:
        closure = ocn.Smagorinsky(coefficient=ocn.DynamicCoefficient(averaging=averaging)) if averaging == 1 else ocn.DynamicSmagorinsky(averaging=averaging)
        model = ocn.NonhydrostaticModel(grid=grid, closure=closure, tracers=())
        K = model.diffusivity_fields
        want = tuple(r or n for r, n in zip(reduced, grid.size))
        assert size(K.𝒥ᴸᴹ) == want and size(K.𝒥ᴹᴹ) == want and size(K.J_LM) == want
        for f in (K.LM, K.MM, K.Σ, K.Σ̄, K.νₑ, K.Sigma, K.Sigma_bar):
            assert size(f) == grid.size
        assert K._fields[1:] == ("Σ", "Σ̄", "LM", "MM", "JLM", "JMM")
        model.close()
    model = ocn.NonhydrostaticModel(grid=grid, closure=ocn.DynamicSmagorinsky(averaging=ocn.LagrangianAveraging()), tracers=())
    K = model.diffusivity_fields
    for f in (K.𝒥ᴸᴹ, K.𝒥ᴹᴹ, K.J_LM_prev, K.J_MM_prev, K.Σ, K.Σ̄):
        assert size(f) == grid.size
    assert not hasattr(K, "LM") and len(K) == 7
    model.close()


def _model(ocn, arch, name, closure, timestepper="RungeKutta3"):
    grid = R.make_grid(ocn, arch, name)
    model = ocn.NonhydrostaticModel(grid=grid, closure=closure, tracers=("T",), timestepper=timestepper)
    vals, _ = R.case_values(grid, "none")
    ocn.set_model(model, T=lambda x, y, z: 20 + 0.0 * (x + y + z), **vals)
    return grid, model


def _model_parents(model):
    return [f.parent() for f in model.velocities]


@pytest.mark.parametrize("name", ["ppp", "bbb"])
def test_directional_model_rk3(ocn, arch, name):
    """after each of 3 steps LM, MM, 𝒥 and νₑ are the restatement evaluated on model.velocities, exactly; the step runs without the graph"""
    dc = ocn.DynamicCoefficient(averaging=(1, 2))
    grid, model = _model(ocn, arch, name, ocn.Smagorinsky(coefficient=dc))
    K = model.diffusivity_fields
    d = R.DynamicDriver(grid, 3)
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    for step in range(3):
        ocn.time_step(model, dt)
        u, v, w = _model_parents(model)
        assert d.update(u, v, w, model.clock.time, model.clock.iteration, model.clock.last_Δt)
        assert np.array_equal(K.Σ.parent(), d.Sigma) and np.array_equal(K.Σ̄.parent(), d.Sigma_bar)
        assert np.array_equal(K.LM.interior(), d.LM) and np.array_equal(K.MM.interior(), d.MM)
        assert np.array_equal(K.J_LM.interior(), d.J_LM) and np.array_equal(K.J_MM.interior(), d.J_MM)
        assert np.array_equal(K.νₑ.interior(), d.viscosity(u, v, w))
        for f in model.fields().values():
            assert np.isfinite(f.parent()).all()
    assert abs(ocn.max_abs_divergence(model)) <= 5e-8                       # the bound of tests/test_gpu_smagorinsky.py
    assert model.get_option("graph_captures") == 0 and model.get_option("graph_replays") == 0
    assert K.νₑ.interior().max() > 0
    model.close()


def test_the_schedule_holds_the_coefficient(ocn, arch):
    """IterationInterval(3) under RK3, whose three updates per step see the iterations (n, n, n + 1) (the truth table of
    test_dynamic_smagorinsky_host.py). Step 1 sees (0, 0, 1): its first two updates fire, on the velocities of stages 1 and 2, and the
    last one does not -- so 𝒥 after step 1 is neither the initial 𝒥 nor the 𝒥 of the step's final velocities, and it is HELD from there:
    unchanged after step 2 (1, 1, 2) and, with that copy, "unchanged after steps 1 and 2"; step 3 (2, 2, 3) fires at its end, so 𝒥 changes
    and is the 𝒥 of the final velocities. Throughout νₑ is viscosity(current velocities, held 𝒥)."""
    dc = ocn.DynamicCoefficient(averaging=(1, 2), schedule=ocn.IterationInterval(3))
    grid, model = _model(ocn, arch, "ppp", ocn.Smagorinsky(coefficient=dc))
    K = model.diffusivity_fields
    m = R.Metrics(grid)
    ocn.update_state(model, True)
    J = lambda: (K.J_LM.interior().copy(), K.J_MM.interior().copy())       # noqa: E731
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])       # noqa: E731
    of_final = lambda: R.DynamicDriver(grid, 3)                             # noqa: E731
    initial = J()
    assert np.abs(initial[1]).min() > 0
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    held = None
    for step in (1, 2, 3):
        ocn.time_step(model, dt)
        now = J()
        u, v, w = _model_parents(model)
        d = of_final()
        d.coefficient_update(u, v, w)
        final = (d.J_LM, d.J_MM)
        if step == 1:
            assert not same(now, initial) and not same(now, final)          # updated at stages 1 and 2 (iteration 0), not at the end
            held = now
        elif step == 2:
            assert same(now, held) and not same(now, final)                 # no update at (1, 1, 2)
        else:
            assert not same(now, held) and same(now, final)                 # the update that ends step 3 (iteration 3)
        assert np.array_equal(K.νₑ.interior(), R.viscosity(m, u, v, w, now[0], now[1], dc.minimum_numerator))
    model.close()


@pytest.mark.parametrize("name", ["ppp", "ppb"])
def test_lagrangian_model_ab2(ocn, arch, name):
    """QuasiAdamsBashforth2 updates the state once per step: the restatement, fed the model's velocities after every step, reproduces 𝒥
    (whole parents) and νₑ exactly"""
    dc = ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging())
    grid, model = _model(ocn, arch, name, ocn.Smagorinsky(coefficient=dc), "QuasiAdamsBashforth2")
    K = model.diffusivity_fields
    d = R.DynamicDriver(grid, 0)
    u, v, w = _model_parents(model)
    d.update(u, v, w, 0.0, 0, np.inf)
    assert np.array_equal(K.J_LM.parent(), d.J_LM) and np.array_equal(K.J_MM.parent(), d.J_MM)     # set! has updated the state
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    for step in range(3):
        ocn.time_step(model, dt)
        u, v, w = _model_parents(model)
        d.update(u, v, w, model.clock.time, model.clock.iteration, model.clock.last_Δt)
        assert np.array_equal(K.J_LM.parent(), d.J_LM) and np.array_equal(K.J_MM.parent(), d.J_MM), step
        assert np.array_equal(K.J_LM_prev.parent(), d.J_LM_prev) and np.array_equal(K.J_MM_prev.parent(), d.J_MM_prev), step
        assert np.array_equal(K.νₑ.interior(), d.viscosity(u, v, w)), step
    assert d.initialisations == 1 and d.updates == 4
    assert model.get_option("graph_captures") == 0
    model.close()


def test_lagrangian_model_rk3(ocn, arch):
    """RK3, 2 steps: 𝒥ᴸᴹ >= minimum_numerator everywhere, νₑ == viscosity(model velocities, device 𝒥), every field finite"""
    dc = ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging(), minimum_numerator=1e-20)
    grid, model = _model(ocn, arch, "ppb", ocn.Smagorinsky(coefficient=dc))
    K = model.diffusivity_fields
    m = R.Metrics(grid)
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    for step in range(2):
        ocn.time_step(model, dt)
    u, v, w = _model_parents(model)
    assert K.J_LM.parent().min() >= 1e-20
    assert np.array_equal(K.νₑ.interior(), R.viscosity(m, u, v, w, K.J_LM.interior(), K.J_MM.interior(), 1e-20))
    for f in list(model.fields().values()) + list(K):
        assert np.isfinite(f.parent()).all()
    interior = K.J_MM.interior()
    assert not np.all(interior == interior[0, 0, 0])                       # the averaging branch has run (the third tick! makes last_Δt finite)
    assert abs(ocn.max_abs_divergence(model)) <= 5e-8
    assert model.get_option("graph_captures") == 0
    model.close()


def test_error_codes(ocn, arch, cases):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    grid, flds, Pn, _ = cases["bbb"]
    dc = ocn.DynamicCoefficient(averaging=(1, 2))
    fields = ocn.kernels.dynamic_coefficient_fields(grid, dc)
    p = lambda n: fields[n].data if n in fields else None                  # noqa: E731
    args = lambda mask: (grid.handle, flds["u"].data, flds["v"].data, flds["w"].data, mask, 1e-32, 0.1, 1, p("Sigma"), p("Sigma_bar"), p("LM"),  # noqa: E731
                         p("MM"), p("J_LM"), p("J_MM"), None, None)
    assert L.ocn_dynamic_smagorinsky_update(*args(3)) == 0
    assert L.ocn_dynamic_smagorinsky_update(*args(8)) == OCN_EINVAL
    assert L.ocn_dynamic_smagorinsky_update(*args(0)) == OCN_EINVAL                 # Lagrangian without the previous fields
    nu = ocn.CenterField(grid)
    assert L.ocn_compute_dynamic_smagorinsky_viscosity(grid.handle, 9, 1e-32, p("J_LM"), p("J_MM"), flds["u"].data, flds["v"].data, flds["w"].data,
                                                       nu.data) == OCN_EINVAL
    assert L.ocn_compute_dynamic_smagorinsky_viscosity(grid.handle, 3, 1e-32, None, p("J_MM"), flds["u"].data, flds["v"].data, flds["w"].data,
                                                       nu.data) == OCN_EINVAL
    # halos below 2
    thin = ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1), halo=(1, 1, 1))
    tf = {n: f(thin) for n, f in (("u", ocn.XFaceField), ("v", ocn.YFaceField), ("w", ocn.ZFaceField))}
    tk = ocn.kernels.dynamic_coefficient_fields(thin, dc)
    assert L.ocn_dynamic_smagorinsky_update(thin.handle, tf["u"].data, tf["v"].data, tf["w"].data, 3, 1e-32, 0.0, 1, tk["Sigma"].data,
                                            tk["Sigma_bar"].data, tk["LM"].data, tk["MM"].data, tk["J_LM"].data, tk["J_MM"].data, None,
                                            None) == OCN_EINVAL and b"halos" in L.ocn_last_error()
    # the model entry
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), closure=ocn.Smagorinsky())
    ptr, loc = C.c_void_p(), (C.c_int * 3)()
    assert L.ocn_model_field(model.handle, b"J_LM", C.byref(ptr), loc) == OCN_ESTATE          # no dynamic coefficient
    pr = (C.c_double * 1)(1.0)
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 8, 1e-32, 1, 0, pr) == OCN_EINVAL
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 3, 1e-32, 0, 0, pr) == OCN_EINVAL
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 3, float("nan"), 1, 0, pr) == OCN_EINVAL
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 3, 1e-32, 1, 0, (C.c_double * 1)(0.0)) == OCN_EINVAL
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 3, 1e-32, 1, 0, pr) == 0
    assert L.ocn_model_field(model.handle, b"J_LM", C.byref(ptr), loc) == 0 and L.ocn_model_field(model.handle, b"LM", C.byref(ptr), loc) == 0
    assert L.ocn_model_field(model.handle, b"J_LM_prev", C.byref(ptr), loc) == OCN_ESTATE     # directional averaging has no 𝒥⁻
    assert L.ocn_model_field(model.handle, b"kappa_e0", C.byref(ptr), loc) == OCN_ESTATE
    assert L.ocn_model_set_dynamic_smagorinsky(model.handle, 0, 1e-32, 1, 0, pr) == 0
    assert L.ocn_model_field(model.handle, b"J_LM_prev", C.byref(ptr), loc) == 0 and L.ocn_model_field(model.handle, b"LM", C.byref(ptr), loc) == OCN_ESTATE
    assert L.ocn_model_set_smagorinsky(model.handle, 0.16, 1.0, 0, pr) == 0                  # a constant coefficient replaces it
    assert L.ocn_model_field(model.handle, b"Sigma", C.byref(ptr), loc) == OCN_ESTATE
    model.close()
    # a Flat direction
    flat = ocn.RectilinearGrid(arch, size=(8, 1, 8), x=(0, 1), y=(0, 1), z=(0, 1), topology=(ocn.Periodic, ocn.Flat, ocn.Periodic))
    plain = ocn.NonhydrostaticModel(grid=flat, tracers=())
    assert L.ocn_model_set_dynamic_smagorinsky(plain.handle, 3, 1e-32, 1, 0, None) == OCN_EINVAL and b"Flat" in L.ocn_last_error()
    with pytest.raises(_lib.OcnError):
        ocn.NonhydrostaticModel(grid=flat, tracers=(), closure=ocn.DynamicSmagorinsky(averaging=1))
    plain.close()


def test_partitioned_handles_refuse_the_dynamic_coefficient(ocn, arch):
    """OCN_ENOTSUP on a partitioned handle (one rank that is its own neighbour); Python refuses before a handle exists"""
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import distributed as dist
    L = _lib.lib()
    uid = C.create_string_buffer(128)
    _lib.check(L.ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    grid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    part = dist.LibraryDistributedModel(grid=grid, tracers=())
    assert L.ocn_model_set_dynamic_smagorinsky(part.handle, 3, 1e-32, 1, 0, None) == OCN_ENOTSUP and b"partitioned" in L.ocn_last_error()
    with pytest.raises(NotImplementedError, match="partitioned"):
        dist.LibraryDistributedModel(grid=grid, tracers=(), closure=ocn.DynamicSmagorinsky(averaging=(1, 2)))
    part.close()
    ctx.close()


@pytest.mark.parametrize("interval", [1, 2])
def test_a_restored_lagrangian_model_initialises_its_average(ocn, arch, tmp_path, interval):
    """the 𝒥 fields are not checkpointed. set!(model, file) sets the clock (time > 0, finite last_Δt) and updates the state: the first update
    that fires takes the initialising branch from the restored velocities, later ones average. 𝒥ᴹᴹ > 0 and νₑ > 0 after a step, and the
    restatement, restarted at the restored clock, reproduces 𝒥 and νₑ exactly. interval 2, restored at iteration 3: the restore's own
    update does not fire, the one that ends the next step does"""
    dc = ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging(), schedule=ocn.IterationInterval(interval))
    grid, first = _model(ocn, arch, "ppp", ocn.Smagorinsky(coefficient=dc), "QuasiAdamsBashforth2")
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    for _ in range(3):
        ocn.time_step(first, dt)
    path = ocn.write_checkpoint(first, str(tmp_path / "dynamic.npz"))
    first.close()
    model = ocn.NonhydrostaticModel(grid=grid, closure=ocn.Smagorinsky(coefficient=dc), tracers=("T",), timestepper="QuasiAdamsBashforth2")
    ocn.set_from_checkpoint(model, path)
    K = model.diffusivity_fields
    assert model.clock.iteration == 3 and model.clock.time > 0 and np.isfinite(model.clock.last_Δt)
    d = R.DynamicDriver(grid, 0, interval=interval)
    d.restart(model.clock.time)
    fired = d.update(*_model_parents(model), model.clock.time, model.clock.iteration, model.clock.last_Δt)
    assert fired == (interval == 1) and d.initialisations == int(fired)
    for step in range(2):
        ocn.time_step(model, dt)
        u, v, w = _model_parents(model)
        d.update(u, v, w, model.clock.time, model.clock.iteration, model.clock.last_Δt)
        assert np.array_equal(K.J_LM.parent(), d.J_LM) and np.array_equal(K.J_MM.parent(), d.J_MM), step
        assert np.array_equal(K.νₑ.interior(), d.viscosity(u, v, w)), step
        assert K.J_MM.interior().min() > 0 and K.νₑ.interior().max() > 0
    assert d.initialisations == 1 and d.updates == (3 if interval == 1 else 1)
    model.close()


def test_lagrangian_averaging_needs_the_grid_s_nodes(ocn, arch, cases):
    """OCN_ESTATE of both entries on a grid that was given neither ocn_grid_set_nodes nor ocn_grid_set_node_tables; directional
    averaging needs neither"""
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    like, flds, Pn, _ = cases["bbb"]                                       # arrays of the same shape (never touched by a refused call)
    raw = C.c_void_p()
    assert L.ocn_grid_create(C.byref(raw), _lib.i3(like.size), _lib.i3(like.halo_size), _lib.i3((1, 1, 1)), (C.c_double * 3)(1.0, 1.0, 1.0),
                             like.Δxᶜᵃᵃ, like.Δyᵃᶜᵃ, like._dz, None, None) == 0
    lag = ocn.kernels.dynamic_coefficient_fields(like, ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging()))
    args = (raw, flds["u"].data, flds["v"].data, flds["w"].data, 0, 1e-32, 0.0, 1, lag["Sigma"].data, lag["Sigma_bar"].data, None, None,
            lag["J_LM"].data, lag["J_MM"].data, lag["J_LM_prev"].data, lag["J_MM_prev"].data)
    assert L.ocn_dynamic_smagorinsky_update(*args) == OCN_ESTATE and b"ocn_grid_set_nodes" in L.ocn_last_error()
    handle = C.c_void_p()
    assert L.ocn_model_create(C.byref(handle), raw, 0) == 0
    assert L.ocn_model_set_dynamic_smagorinsky(handle, 0, 1e-32, 1, 0, None) == OCN_ESTATE and b"ocn_grid_set_nodes" in L.ocn_last_error()
    assert L.ocn_model_set_dynamic_smagorinsky(handle, 3, 1e-32, 1, 0, None) == 0
    assert L.ocn_model_destroy(handle) == 0 and L.ocn_grid_destroy(raw) == 0
