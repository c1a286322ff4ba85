"""Smagorinsky / SmagorinskyLilly on the MI355X: the eddy-viscosity kernels bit for bit against the numpy restatement
(tests/smagorinsky_reference.py, pinned by analytic known answers in tests/test_smagorinsky_host.py) and against each other, the tracer
coefficient ℑ(νₑ) / Pr against the oracle's array-coefficient closure term, the model's tendencies, the step paths, the reference's
data-free closure checks and the partitioned step."""
import ctypes as C

import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import smagorinsky_reference as R

pytestmark = pytest.mark.gpu

CENTER, FACE = 0, 1
OCN_EINVAL, OCN_ESTATE = -1, -3          # include/ocn_mi355x.h
ORO_LOC = {"u": (FACE, CENTER, CENTER), "v": (CENTER, FACE, CENTER), "w": (CENTER, CENTER, FACE)}


def _fields(ocn, grid, vals):
    """device fields of a case's interior values with filled halos -> (dict name -> Field, dict name -> parent array)"""
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds = {n: make.get(n, ocn.CenterField)(grid).set(v) for n, v in vals.items()}
    ocn.fill_halo_regions(list(flds.values()))
    return flds, {n: f.parent() for n, f in flds.items()}


def _buoyancy(ocn, kind):
    if kind == "none":
        return None
    if kind == "tracer":
        return ocn.BuoyancyTracer()
    return ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=R.ALPHA, haline_contraction=R.BETA), gravitational_acceleration=R.GRAV)


def _interior(grid, a):
    return a[grid.Hx:grid.Hx + grid.Nx, grid.Hy:grid.Hy + grid.Ny, grid.Hz:grid.Hz + grid.Nz]


def _both_kernels(ocn, grid, closure, buoyancy, flds, rng=None):
    """νₑ by the marching kernel (the default) and by the per-cell kernel -> two parent arrays"""
    out = []
    try:
        for march in (1, 0):
            ocn.set_option("smag_march", march)
            nu = ocn.CenterField(grid)
            ocn.kernels.compute_smagorinsky_viscosity(grid, closure, buoyancy, flds, flds["u"], flds["v"], flds["w"], nu, kernel_parameters=rng)
            out.append(nu.parent())
    finally:
        ocn.set_option("smag_march", 1)
    return out


VARIANTS = [("constant", "none", None)] + [("lilly", kind, Cb) for kind, Cb in R.LILLY_CASES]


@pytest.mark.parametrize("variant,kind,Cb", VARIANTS)
@pytest.mark.parametrize("name", list(R.GRIDS))
def test_eddy_viscosity_is_the_restatement_bit_for_bit(ocn, arch, name, variant, kind, Cb):
    """both kernels == the restatement and == each other; the Lilly cases with buoyancy have >= 10 % of their cells in each regime of ς"""
    grid = R.make_grid(ocn, arch, name)
    vals, _ = R.case_values(grid, kind)
    flds, P = _fields(ocn, grid, vals)
    m = R.Metrics(grid)
    closure = ocn.Smagorinsky(coefficient=0.16) if variant == "constant" else ocn.SmagorinskyLilly(C=0.16, Cb=Cb)
    want = R.viscosity(m, P["u"], P["v"], P["w"], 0.16, Cb=Cb, buoyancy=R.buoyancy_of(kind, P))
    assert want.max() > 0 and not np.isnan(want).any()
    if variant == "lilly" and kind != "none":
        assert min(R.regime_fractions(m, P["u"], P["v"], P["w"], Cb, R.buoyancy_of(kind, P))) >= 0.10
    march, cell = _both_kernels(ocn, grid, closure, _buoyancy(ocn, kind), flds)
    assert np.array_equal(_interior(grid, cell), want), ("per-cell kernel", np.abs(_interior(grid, cell) - want).max())
    assert np.array_equal(_interior(grid, march), want), ("marching kernel", np.abs(_interior(grid, march) - want).max())
    assert np.array_equal(march, cell)                     # (halos: both leave the zeros of the allocation)


def test_eddy_viscosity_in_the_halo_columns(ocn, arch):
    """range = {0, Nx + 1, 0, Ny + 1, 1, Nz}: what a pencil rank computes from exchanged halos"""
    grid = R.make_grid(ocn, arch, "ppp")
    vals, _ = R.case_values(grid, "seawater")
    flds, P = _fields(ocn, grid, vals)
    rng = (0, grid.Nx + 1, 0, grid.Ny + 1, 1, grid.Nz)
    want = R.viscosity(R.Metrics(grid), P["u"], P["v"], P["w"], 0.16, Cb=1.0, buoyancy=R.buoyancy_of("seawater", P), rng=rng)
    for got in _both_kernels(ocn, grid, ocn.SmagorinskyLilly(), _buoyancy(ocn, "seawater"), flds, rng=rng):
        H = grid.Hx
        assert np.array_equal(got[H - 1:H + grid.Nx + 1, H - 1:H + grid.Ny + 1, H:H + grid.Nz], want)
        got[H - 1:H + grid.Nx + 1, H - 1:H + grid.Ny + 1, H:H + grid.Nz] = 0.0
        assert not got.any()                               # nothing outside the range is written
    from oldoceananigans_jl_amd import _lib
    nu = ocn.CenterField(grid)
    with pytest.raises(_lib.OcnError):                     # H - 1 cells into the halos at most
        ocn.kernels.compute_smagorinsky_viscosity(grid, ocn.Smagorinsky(), None, flds, flds["u"], flds["v"], flds["w"], nu,
                                                  kernel_parameters=(-2, grid.Nx, 1, grid.Ny, 1, grid.Nz))


@pytest.mark.parametrize("spacing", [1.0, 2.0])
def test_known_answers_on_the_device(ocn, arch, spacing):
    """the analytic answers of test_smagorinsky_host.py in the interior of Bounded 6³ grids of spacing 1 and 2 (rtol 1e-13)"""
    L = 6.0 * spacing
    grid = ocn.RectilinearGrid(arch, size=(6, 6, 6), x=(0.0, L), y=(0.0, L), z=(-L, 0.0), topology=(ocn.Bounded,) * 3, halo=(3, 3, 3))
    Cs, df2 = 0.16, spacing * spacing
    inner = (slice(4, 8),) * 3          # cells 2 .. 5: their stencils stay inside the analytic interior values

    def run(closure, buoyancy, **fn):
        names = ["u", "v", "w"] + (["b"] if isinstance(buoyancy, ocn.BuoyancyTracer) else [])
        make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
        flds = {}
        for n in names:
            f = make.get(n, ocn.CenterField)(grid)
            x, y, z = [np.asarray(a, dtype=np.float64) for a in (
                (grid.xᶠᵃᵃ if n == "u" else grid.xᶜᵃᵃ)[:, None, None], (grid.yᵃᶠᵃ if n == "v" else grid.yᵃᶜᵃ)[None, :, None],
                (grid.zᵃᵃᶠ if n == "w" else grid.zᵃᵃᶜ)[None, None, :])]
            f.set_parent(np.broadcast_to(fn[n](x, y, z) if n in fn else 0.0 * (x + y + z), f.shape))       # analytic in the halos too
            flds[n] = f
        full = _both_kernels(ocn, grid, closure, buoyancy, flds)
        return [a[inner] for a in full], full

    for S in (0.7, -1.3):
        for got in run(ocn.Smagorinsky(coefficient=Cs), None, u=lambda x, y, z: S * z + 0.0 * (x + y))[0]:
            assert np.allclose(got, Cs * Cs * df2 * abs(S), rtol=1e-13, atol=0.0)
    for closure in (ocn.Smagorinsky(coefficient=Cs), ocn.SmagorinskyLilly(C=Cs)):
        for got in run(closure, None, u=lambda x, y, z: x + 0.0 * (y + z), v=lambda x, y, z: y + 0.0 * (x + z), w=lambda x, y, z: -2.0 * z + 0.0 * (x + y))[0]:
            assert np.allclose(got, Cs * Cs * df2 * np.sqrt(12.0), rtol=1e-13, atol=0.0)
    for closure, buoyancy in ((ocn.Smagorinsky(coefficient=Cs), None), (ocn.SmagorinskyLilly(C=Cs), None), (ocn.SmagorinskyLilly(C=Cs), ocn.BuoyancyTracer())):
        for got in run(closure, buoyancy, b=lambda x, y, z: 0.3 * z + 0.0 * (x + y))[1]:                  # fluid at rest: +0.0, no NaN anywhere
            assert not np.isnan(got).any() and np.all(got == 0.0) and not np.signbit(got).any()
    S = 1.1
    shear = lambda x, y, z: S * z + 0.0 * (x + y)          # noqa: E731
    unstratified = run(ocn.SmagorinskyLilly(C=Cs), None, u=shear)[0]
    for N2 in (0.1, 0.4):
        for got in run(ocn.SmagorinskyLilly(C=Cs, Cb=1.0), ocn.BuoyancyTracer(), u=shear, b=lambda x, y, z: N2 * z + 0.0 * (x + y))[0]:
            assert np.allclose(got, Cs * Cs * df2 * S * np.sqrt(1 - 2 * N2 / (S * S)), rtol=1e-13, atol=0.0)
    for N2 in (S * S, 5.0):
        for got in run(ocn.SmagorinskyLilly(C=Cs, Cb=1.0), ocn.BuoyancyTracer(), u=shear, b=lambda x, y, z: N2 * z + 0.0 * (x + y))[0]:
            assert np.all(got == 0.0)
    for got, ref in zip(run(ocn.SmagorinskyLilly(C=Cs, Cb=1.0), ocn.BuoyancyTracer(), u=shear, b=lambda x, y, z: -0.8 * z + 0.0 * (x + y))[0], unstratified):
        assert np.array_equal(got, ref)


def _oracle_grid(oracle, name):
    c = R.GRIDS[name]
    z = tanh_faces(c["size"][2]) if c["stretched"] else ((-1.0, 0.0) if c["topology"][2] == "B" else (0.0, 1.0))
    return oracle.Grid(c["size"], topology=tuple({"P": 0, "B": 1}[t] for t in c["topology"]), x=(0.0, 1.0), y=(0.0, 1.0), z=z)


def _oracle_closure_term(oracle, g, which, P, c, coef, G):
    """G = (G - closure term) + 0 with the coefficient array `coef` (ccc, halos filled), by the oracle"""
    G = np.asfortranarray(G.copy())
    dp = C.POINTER(C.c_double)
    ptr = lambda a: np.asfortranarray(a).ctypes.data_as(dp)          # noqa: E731
    keep = [np.asfortranarray(a) for a in (P["u"], P["v"], P["w"], c if c is not None else P["u"], coef)]
    oracle.lib().oro_add_closure_tendency_field(g.handle, which, *[a.ctypes.data_as(dp) for a in keep], G.ctypes.data_as(dp), None)
    return G


@pytest.mark.parametrize("name", ["ppb", "bbb"])
def test_tracer_coefficient_is_the_interpolated_viscosity_over_pr(ocn, oracle, arch, name):
    """Pr = 1 == the array-coefficient entry point with κₑ = νₑ == the oracle; Pr = 2 == the oracle with νₑ / 2 (exact scaling);
    Pr = {T: 1, S: 3} == the restatement's ∇·q and within 1e-12 of the oracle with νₑ / 3; momentum == the oracle in every case"""
    grid = R.make_grid(ocn, arch, name)
    g_cpu = _oracle_grid(oracle, name)
    vals, names = R.case_values(grid, "seawater")
    flds, P = _fields(ocn, grid, vals)
    m = R.Metrics(grid)
    nu = ocn.CenterField(grid)
    ocn.kernels.compute_smagorinsky_viscosity(grid, ocn.SmagorinskyLilly(), _buoyancy(ocn, "seawater"), flds, flds["u"], flds["v"], flds["w"], nu)
    ocn.fill_halo_regions([nu])
    nu_h = nu.parent()
    order = ["u", "v", "w", "T", "S"]
    rng = np.random.default_rng(5)
    G0 = {n: np.asfortranarray(rng.standard_normal(flds[n].shape)) for n in order}          # "the advective part"

    def product(entry, closure=None, G0=G0):
        G = {n: type(flds[n])(flds[n].loc, grid) for n in order}
        for n in order:
            G[n].set_parent(G0[n])
        if entry == "field":
            ocn.kernels.compute_closure_tendencies_field(grid, [flds[n] for n in order], [G[n] for n in order], nu, [nu, nu])
        else:
            ocn.kernels.compute_closure_tendencies_smagorinsky(grid, [flds[n] for n in order], [G[n] for n in order], nu, closure, names)
        return {n: G[n].parent() for n in order}

    def oracle_terms(pr):
        out = {n: _oracle_closure_term(oracle, g_cpu, w, P, None, nu_h, G0[n]) for w, n in enumerate(("u", "v", "w"))}
        for n in ("T", "S"):
            out[n] = _oracle_closure_term(oracle, g_cpu, 3, P, P[n], nu_h / pr[n], G0[n])
        return out

    one = product("smagorinsky", ocn.Smagorinsky(Pr=1.0))
    fld = product("field")
    ref = oracle_terms({"T": 1.0, "S": 1.0})
    for n in order:
        assert np.array_equal(one[n], fld[n]) and np.array_equal(one[n], ref[n]), n
        assert not np.array_equal(one[n], G0[n]), n
    two = product("smagorinsky", ocn.Smagorinsky(Pr=2.0))
    ref = oracle_terms({"T": 2.0, "S": 2.0})
    for n in order:
        assert np.array_equal(two[n], ref[n]), n
    mixed = product("smagorinsky", ocn.SmagorinskyLilly(Pr={"T": 1.0, "S": 3.0}))
    ref = oracle_terms({"T": 1.0, "S": 3.0})
    for n in ("u", "v", "w", "T"):
        assert np.array_equal(mixed[n], ref[n]), n
    want = (_interior(grid, G0["S"]) - R.div_q(m, P["S"], nu_h, 3.0)) + 0.0
    assert np.array_equal(_interior(grid, mixed["S"]), want)
    # the closure term alone (added to zero, so that the random "advective part" does not mask it) against the oracle's with κ = νₑ / 3
    Z = {n: np.zeros_like(G0[n]) for n in order}
    term = product("smagorinsky", ocn.SmagorinskyLilly(Pr={"T": 1.0, "S": 3.0}), G0=Z)["S"]
    err = rel_err(_interior(grid, term), _interior(grid, _oracle_closure_term(oracle, g_cpu, 3, P, P["S"], nu_h / 3.0, Z["S"])))
    assert np.abs(term).max() > 0
    print("Pr = 3: closure term vs oracle with nu_e / 3:", err)
    assert err <= 1e-12


def _physics_model(ocn, arch, closure, timestepper="RungeKutta3", seed=1234):
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 12), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(12), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    F = ocn.FieldBoundaryConditions
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=closure, coriolis=ocn.FPlane(f=0.3), timestepper=timestepper,
                                    buoyancy=_buoyancy(ocn, "seawater"),
                                    boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-3)), "T": F(top=ocn.FluxBoundaryCondition(4e-3))})
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed)
    vals["T"] = vals["T"] + (R.STRATIFICATION["seawater"] / (R.GRAV * R.ALPHA)) * grid.nodes((ocn.Center,) * 3)[2]
    ocn.set_model(model, **vals)
    return grid, model


def test_model_tendencies_are_the_oracle_pieces(ocn, oracle, arch):
    """after update_state!: the model's νₑ (halos included) == restatement + fill, and Gⁿ of every field == ((advective G - Coriolis) -
    hydrostatic gradient) - closure term assembled from the oracle's pieces with that νₑ"""
    grid, model = _physics_model(ocn, arch, ocn.SmagorinskyLilly())
    ocn.update_state(model, True)
    P = {n: f.parent() for n, f in model.fields().items()}
    m = R.Metrics(grid)
    want = ocn.CenterField(grid)
    want.set(R.viscosity(m, P["u"], P["v"], P["w"], 0.16, Cb=1.0, buoyancy=("seawater", P["T"], P["S"], R.GRAV, R.ALPHA, R.BETA)))
    ocn.fill_halo_regions([want])
    nu_h = model.diffusivity_fields.νₑ.parent()
    assert np.array_equal(nu_h, want.parent()) and nu_h.max() > 0
    g = oracle.Grid((16, 16, 12), topology=(0, 0, 1), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(12))
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)          # noqa: E731
    u, v, w, T, S = [np.asfortranarray(P[n]) for n in ("u", "v", "w", "T", "S")]
    G = {}
    for n in ("u", "v", "w"):
        G[n] = g.zeros(ORO_LOC[n])
        g.compute_G(n, u, v, w, G[n])
    for n, c in (("T", T), ("S", S)):
        G[n] = g.zeros((0, 0, 0))
        g.compute_G("c", u, v, w, G[n], c=c)
    L = oracle.lib()
    L.oro_add_fplane_coriolis.argtypes = [C.c_void_p, C.c_double, dp, dp, dp, dp]
    L.oro_add_fplane_coriolis(g.handle, 0.3, ptr(u), ptr(v), ptr(G["u"]), ptr(G["v"]))
    pHY = g.zeros((0, 0, 0))
    L.oro_update_hydrostatic_pressure(g.handle, 2, ptr(T), ptr(S), R.GRAV, R.ALPHA, R.BETA, ptr(pHY))
    L.oro_add_hydrostatic_pressure_gradient(g.handle, ptr(pHY), ptr(G["u"]), ptr(G["v"]))
    for which, n in enumerate(("u", "v", "w")):
        G[n] = _oracle_closure_term(oracle, g, which, P, None, nu_h, G[n])
    for n, c in (("T", T), ("S", S)):
        G[n] = _oracle_closure_term(oracle, g, 3, P, c, nu_h, G[n])
    for n in ("u", "v", "w", "T", "S"):
        got = model.tendency(n).parent()
        sl = tuple(slice(3, 3 + k) for k in grid.interior_size(model.fields()[n].loc))
        assert np.array_equal(got[sl], G[n][sl]), (n, np.abs(got[sl] - G[n][sl]).max())


@pytest.mark.parametrize("Pr", [1.0, {"T": 1.0, "S": 3.0}], ids=["Pr1", "PrTS"])
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_step_paths_agree_bitwise(ocn, arch, timestepper, Pr):
    """defaults (fused marching epilogue, marching νₑ kernel, fused substep) against every one of them switched off, after 3 steps"""
    models = []
    for plain in (False, True):
        grid, model = _physics_model(ocn, arch, ocn.SmagorinskyLilly(Pr=Pr), timestepper)
        if plain:
            for key in ("fused_epilogue", "epilogue_march", "smag_march", "fuse_substep"):
                model.set_option(key, 0)
        models.append(model)
    dt = 0.1 * float(np.min(grid.Δzᵃᵃᶜ)) / 0.6
    for _ in range(3):
        for model in models:
            ocn.time_step(model, dt)
    a, b = models
    assert a.clock.time == b.clock.time and a.clock.iteration == 3
    for n in a.fields():
        assert np.array_equal(a.fields()[n].parent(), b.fields()[n].parent()), n
        assert np.isfinite(a.fields()[n].parent()).all()
    assert np.array_equal(a.diffusivity_fields.νₑ.parent(), b.diffusivity_fields.νₑ.parent())
    assert np.array_equal(a.pressures.pNHS.parent(), b.pressures.pNHS.parent())
    if isinstance(Pr, dict):             # the Prandtl number really acts: S differs from a unit-Pr run
        _, unit = _physics_model(ocn, arch, ocn.SmagorinskyLilly(), timestepper)
        for _ in range(3):
            ocn.time_step(unit, dt)
        assert not np.array_equal(unit.tracers.S.parent(), a.tracers.S.parent())


@pytest.mark.parametrize("which", ["Smagorinsky", "SmagorinskyLilly"])
def test_time_stepping_works_with_closure(ocn, arch, which):
    """time_stepping_works_with_closure (test_time_stepping.jl:243-256 runs it for both): a step leaves finite fields; νₑ >= 0; and
    max |∇·u| after 10 steps within the bound of test_incompressibility"""
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), extent=(1, 2, 3), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    closure = getattr(ocn, which)()
    model = ocn.NonhydrostaticModel(grid=grid, closure=closure, tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy())
    rng = np.random.default_rng(3)
    ocn.set_model(model, u=0.1 * rng.standard_normal(grid.interior_size((ocn.Face, ocn.Center, ocn.Center))),
                  v=0.1 * rng.standard_normal(grid.interior_size((ocn.Center, ocn.Face, ocn.Center))), T=lambda x, y, z: 20 + 0.01 * z + 0.0 * (x + y))
    ocn.time_step(model, 1e-3)
    for n, f in model.fields().items():
        assert np.isfinite(f.parent()).all(), n
    for _ in range(9):
        ocn.time_step(model, 1e-3)
    assert abs(ocn.max_abs_divergence(model)) <= 5e-8
    nu = model.diffusivity_fields.νₑ.parent()
    assert np.isfinite(nu).all() and nu.min() >= 0.0 and nu.max() > 0.0
    assert len(model.diffusivity_fields) == 1


def test_a_random_flow_loses_energy_faster_with_the_closure(ocn, arch):
    energies = []
    for closure in (None, ocn.Smagorinsky(), ocn.SmagorinskyLilly()):
        grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), extent=(1, 1, 1))
        model = ocn.NonhydrostaticModel(grid=grid, closure=closure, tracers=())
        rng = np.random.default_rng(11)
        ocn.set_model(model, **{n: rng.standard_normal((16, 16, 16)) for n in "uvw"})
        e0 = sum(float(np.sum(f.interior() ** 2)) for f in model.velocities)
        for _ in range(10):
            ocn.time_step(model, 2e-3)
        energies.append(sum(float(np.sum(f.interior() ** 2)) for f in model.velocities) / e0)
    assert energies[1] < energies[0] < 1.0 and energies[2] < energies[0], energies
    assert energies[1] == energies[2]          # without buoyancy the Lilly coefficient is the constant one (ς = 1)


@pytest.mark.parametrize("case", ["slabs_no_slip", "pencils_pr"])
def test_partitions_match_the_single_gpu_model(ocn, arch, monkeypatch, case):
    """the "amd" preset of test_gpu_dist_library.py with SmagorinskyLilly in place of the AMD closure: four x-slabs of (32, 12, 10) with a
    no-slip bottom (νₑ in the rank-edge z-halo column), and (2, 2) pencils of (16, 12, 8) with a Pr ≠ 1; 1e-12 against the single-GPU
    model, the clock =="""
    import test_gpu_dist_library as me
    pr = 1.0 if case == "slabs_no_slip" else {"T": 1.0, "S": 2.0}
    monkeypatch.setattr(me, "_closure", lambda ocn_, zkind: ocn_.SmagorinskyLilly(C=0.16, Cb=1.0, Pr=pr))
    if case == "slabs_no_slip":
        base = me._bcs

        def no_slip(ocn_, zkind):
            b = dict(base(ocn_, zkind))
            F = ocn_.FieldBoundaryConditions
            b["u"] = F(top=ocn_.FluxBoundaryCondition(-1e-4), bottom=ocn_.ValueBoundaryCondition(0.0))
            b["v"] = F(bottom=ocn_.ValueBoundaryCondition(0.0))
            return b
        monkeypatch.setattr(me, "_bcs", no_slip)
        R_, size, partition = 4, (32, 12, 10), None
    else:
        R_, size, partition = 4, (16, 12, 8), (2, 2)
    me._own_stream()
    nsteps = 3
    results = me._run_library_ranks(ocn, arch, R_, size, nsteps, "amd", {}, partition=partition)
    ref, time, _ = me._single_gpu(ocn, arch, size, "amd", nsteps)
    for r, (out, div, t, off) in enumerate(results):
        assert div < 5e-8 and t == time
        if partition is None:
            me._compare(out, ref, r, size[0] // R_, size)
        else:
            me._compare(out, ref, r, None, size, offset=off[0], joffset=off[1])


def test_diffusion_timescale_and_refusals(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    grid, model = _physics_model(ocn, arch, ocn.SmagorinskyLilly(Pr={"T": 1.0, "S": 0.5}))
    ocn.update_state(model, True)
    nu_max = float(model.diffusivity_fields.νₑ.parent().max())
    delta = min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.min(grid.Δzᵃᵃᶜ[grid.Hz:grid.Hz + grid.Nz])))
    assert ocn.cell_diffusion_timescale(model) == delta ** 2 / max(nu_max, nu_max / 0.5)
    # "kappa_e*" does not exist on a Smagorinsky model; "nu_e" takes boundary conditions
    L = _lib.lib()
    p, loc = C.c_void_p(), (C.c_int * 3)()
    assert L.ocn_model_field(model.handle, b"kappa_e0", C.byref(p), loc) == OCN_ESTATE
    assert L.ocn_model_set_boundary_condition(model.handle, b"kappa_e0", 4, 2, 0.0) == OCN_ESTATE
    assert L.ocn_model_set_boundary_condition(model.handle, b"nu_e", 4, 2, 0.0) == 0
    pr = (C.c_double * 2)(1.0, 1.0)
    assert L.ocn_model_set_smagorinsky(model.handle, -0.1, 1.0, 1, pr) == OCN_EINVAL
    assert L.ocn_model_set_smagorinsky(model.handle, 0.16, 1.0, 1, (C.c_double * 2)(1.0, 0.0)) == OCN_EINVAL
    assert L.ocn_model_set_smagorinsky(model.handle, 0.16, 1.0, 0, pr) == 0
    # replaces an AMD closure: its κₑ fields are gone from the interface
    amd = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.AnisotropicMinimumDissipation())
    assert L.ocn_model_field(amd.handle, b"kappa_e0", C.byref(p), loc) == 0
    assert L.ocn_model_set_smagorinsky(amd.handle, 0.16, 1.0, 1, pr) == 0
    assert L.ocn_model_field(amd.handle, b"kappa_e0", C.byref(p), loc) == OCN_ESTATE
    # a Flat direction
    flat = ocn.RectilinearGrid(arch, size=(8, 1, 8), x=(0, 1), y=(0, 1), z=(0, 1), topology=(ocn.Periodic, ocn.Flat, ocn.Periodic))
    plain = ocn.NonhydrostaticModel(grid=flat, tracers=())
    assert L.ocn_model_set_smagorinsky(plain.handle, 0.16, 1.0, 0, None) == OCN_EINVAL
    with pytest.raises(_lib.OcnError):
        ocn.NonhydrostaticModel(grid=flat, tracers=(), closure=ocn.Smagorinsky())
    with pytest.raises(NotImplementedError):
        ocn.NonhydrostaticModel(grid=grid, closure=(ocn.SmagorinskyLilly(), ocn.ScalarDiffusivity(ν=1e-3)))
    with pytest.raises(NotImplementedError):
        ocn.SmagorinskyLilly(C=ocn.DynamicCoefficient())
    with pytest.raises(ValueError):
        ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.Smagorinsky(Pr={"T": 1.0}))
    with pytest.raises(ValueError):
        ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.Smagorinsky(),
                                boundary_conditions={"κₑ": {"T": ocn.FieldBoundaryConditions(bottom=ocn.ValueBoundaryCondition(0.0))}})
    assert model.get_option("smag_march") == 1
