"""background_fields on the MI355X against the numpy restatement (tests/background_reference.py, pinned to the oracle on the CPU by
tests/test_background_host.py):
  * ocn_compute_advective_tendency == the restatement with advecting != advected, both kernels (per-field, split role), accumulate 0 / 1,
    launch ranges, parent entries outside the range keeping their bits; == ocn_compute_tendencies when advecting ≡ advected;
  * the total velocities == u + Ū over the whole parent array;
  * the model (RK3 and AB2) against the orchestrated yardstick with the new term exercised among all the others, 1e-12;
  * all-zero backgrounds == no backgrounds; cell_advection_timescale and TimeStepWizard on the totals;
  * the reference's data-free arms ("Background fields" of test_dynamics.jl:713-730, time_stepping_with_background_fields);
  * the captured (graph) step of a background model == the uncaptured one."""
import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import background_reference as B
import vertically_implicit_reference as R

pytestmark = pytest.mark.gpu

# (70, 9, 13) PPB stretched: two x tiles with a ragged tail, two row tiles at OCN_ROLE_TY = 7, Nz no multiple of the z chunk; PPP;
# BBB: the per-field path with the wall fall-backs; (Periodic, Flat, Bounded); a two-cell y (reduced-order schemes)
GRIDS = {
    "ppb_stretched": dict(size=(70, 9, 13), topo="PPB", stretched=True),
    "ppp": dict(size=(16, 16, 16), topo="PPP", stretched=False),
    "bbb": dict(size=(12, 10, 8), topo="BBB", stretched=False),
    "pfb": dict(size=(66, 16), topo="PFB", stretched=False),
    "two_cell_y": dict(size=(16, 2, 8), topo="PPB", stretched=False),
}
ROLE_GRIDS = ("ppb_stretched", "ppp")
TRIMMED = (3, 68, 2, 8, 2, 12)


def _grid(ocn, arch, name):
    c = GRIDS[name]
    topo = tuple({"P": ocn.Periodic, "B": ocn.Bounded, "F": ocn.Flat}[t] for t in c["topo"])
    Nz = c["size"][-1]
    kw = dict(z=tanh_faces(Nz) if c["stretched"] else ((-1.0, 0.0) if c["topo"][2] == "B" else (0.0, 1.0)))
    if topo[0] is not ocn.Flat:
        kw["x"] = (0.0, 1.0)
    if topo[1] is not ocn.Flat:
        kw["y"] = (0.0, 1.0)
    return ocn.RectilinearGrid(arch, size=c["size"], topology=topo, **kw)


def _random_fields(ocn, grid, seed, names="uvwc"):
    """random values in the WHOLE parent array -> (dict name -> Field, dict name -> parent array)"""
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}
    flds, parents = {}, {}
    for n in names:
        f = make[n](grid)
        a = np.asfortranarray(rng.standard_normal(f.shape))
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


@pytest.fixture
def tendency_impl(ocn):
    """sets the library default of tendency_impl (what the raw entry points and new models read) and restores it"""
    def set_(v):
        ocn.set_option("tendency_impl", v)
    yield set_
    ocn.set_option("tendency_impl", 2)


CASES = [(n, impl) for n in GRIDS for impl in ((0, 2) if n in ROLE_GRIDS else (2,))]


@pytest.mark.parametrize("name,impl", CASES, ids=[f"{n}-impl{i}" for n, i in CASES])
def test_raw_entry_point_is_the_restatement(ocn, arch, tendency_impl, name, impl):
    """advecting (ua, va, wa) and advected psi are different random arrays: G == -div + 0.0, and with accumulate a pre-filled G == G - div,
    for u, v, w and a tracer; outside the launch range the parent array keeps its bits"""
    tendency_impl(impl)
    grid = _grid(ocn, arch, name)
    m = R.Metrics.of_grid(grid)
    # which kernel serves this grid under this option: asked of a model on the same grid (it copies the library defaults)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("c",), background_fields={"c": 1.0})
    path = model.get_option("background_tendency_path")
    assert model.get_option("background_fields") == 1
    assert path == (2 if (name in ROLE_GRIDS and impl == 2) else 1)
    model.close()
    adv, A = _random_fields(ocn, grid, 41, "uvw")
    psi, P = _random_fields(ocn, grid, 42)
    ranges = [None] + ([TRIMMED] if name == "ppb_stretched" else [])
    for rng in ranges:
        for n in "uvwc":
            for accumulate in (False, True):
                G, G0 = _random_fields(ocn, grid, 43, n)
                ocn.kernels.compute_advective_tendency(grid, adv["u"], adv["v"], adv["w"], psi[n], n, G[n], kernel_parameters=rng,
                                                       accumulate=accumulate)
                want = B.advective_tendency(m, n, (A["u"], A["v"], A["w"]), P[n], rng=rng, G=G0[n].copy(order="F"), accumulate=accumulate)
                got = G[n].parent()
                assert np.array_equal(got, want), (n, rng, accumulate, np.abs(got - want).max())
                assert not np.array_equal(got, G0[n])
                r = m.default_range(R.LOCS[n], n != "c") if rng is None else rng
                inside = np.zeros(got.shape, dtype=bool)
                B._window(m, inside, r)[...] = True
                assert np.array_equal(got[~inside], G0[n][~inside])


@pytest.mark.parametrize("name,impl", CASES, ids=[f"{n}-impl{i}" for n, i in CASES])
def test_advecting_equal_to_advected_is_compute_tendencies(ocn, arch, tendency_impl, name, impl):
    tendency_impl(impl)
    grid = _grid(ocn, arch, name)
    f, _ = _random_fields(ocn, grid, 51)
    Ga, _ = _random_fields(ocn, grid, 52)
    Gb, _ = _random_fields(ocn, grid, 52)
    ocn.kernels.compute_tendencies(grid, f["u"], f["v"], f["w"], [f["c"]], Ga["u"], Ga["v"], Ga["w"], [Ga["c"]])
    for n in "uvwc":
        ocn.kernels.compute_advective_tendency(grid, f["u"], f["v"], f["w"], f[n], n, Gb[n])
        assert np.array_equal(Gb[n].parent(), Ga[n].parent()), n


def test_total_velocities(ocn, arch):
    """after update_state! total_u == u + Ū over the whole parent array, halos included; a component without a background has no total (the
    model's own array advects) and ocn_model_field says so"""
    grid = _grid(ocn, arch, "ppb_stretched")
    ub = ocn.XFaceField(grid)
    ub.set_parent(np.asfortranarray(np.random.default_rng(3).standard_normal(ub.shape)))
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), background_fields={"u": ub, "w": lambda x, y, z: 0.1 * x + 0 * y + z})
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items() if n != "b"}, 5)
    ocn.set_model(model, **vals)
    ocn.update_state(model)
    for n in ("u", "w"):
        U, Ubar = model.fields()[n].parent(), getattr(model.background_fields.velocities, n).parent()
        assert np.array_equal(model._field("total_" + n).parent(), U + Ubar) and np.abs(Ubar).max() > 0
        assert np.array_equal(model._field("bg_" + n).parent(), Ubar)
    assert model.background_fields.velocities.v is None and model.background_fields.tracers.b is None
    for name in ("total_v", "bg_v", "bg_c0"):
        with pytest.raises(ocn.OcnError, match="no background field"):
            model._field(name)
    assert model.get_option("background_fields") == 2 and model.get_option("fuse_substep_active") == 0
    # the standalone sum
    out = ocn.XFaceField(grid)
    ocn.kernels.sum_parent(grid, model.velocities.u, ub, out)
    assert np.array_equal(out.parent(), model.velocities.u.parent() + ub.parent())
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA = 2e-3, {"b": 5e-3, "S": 1e-3}
N2, THETA, FCOR = 0.8, 0.3, 0.7
MODEL_GRIDS = {"ppb_stretched": ((16, 16, 12), ("Periodic", "Periodic", "Bounded"), True), "bbb": ((12, 10, 8), ("Bounded",) * 3, False)}


def _model_pair(ocn, oracle, arch, name, timestepper, forced=True):
    size, topology, stretched = MODEL_GRIDS[name]
    z = tanh_faces(size[2]) if stretched else (-1.0, 0.0)
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=tuple(getattr(ocn, t) for t in topology))
    g_cpu = oracle.Grid(size, topology=tuple(int(t == "Bounded") for t in topology), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    F = ocn.FieldBoundaryConditions
    # u: a shear in z (a function); v: a smooth Field; b: N² (x sinθ + z cosθ), not periodic along the Periodic x; S: none
    U_bg = lambda x, y, z: 0.3 * np.tanh(4 * (z + 0.5)) + 0 * x + 0 * y                    # noqa: E731
    B_bg = lambda x, y, z: N2 * (x * np.sin(THETA) + z * np.cos(THETA)) + 0 * y            # noqa: E731
    vbar = ocn.YFaceField(grid)
    from oldoceananigans_jl_amd.background_fields import parent_nodes
    xv, yv, zv = parent_nodes(grid, vbar.loc)
    vbar.set_parent(np.asfortranarray(0.2 * np.cos(2 * np.pi * xv) * np.sin(2 * np.pi * zv) + 0 * yv))
    forcing = 0.1 * np.random.default_rng(4).standard_normal(size)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b", "S"), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=FCOR),
                                    closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA), forcing={"S": forcing} if forced else None,
                                    boundary_conditions={"b": F(top=ocn.ValueBoundaryCondition(0.4)), "S": F(bottom=ocn.FluxBoundaryCondition(0.03))},
                                    background_fields={"u": U_bg, "v": vbar, "b": ocn.BackgroundField(B_bg)})
    bgf = model.background_fields
    background = {"u": bgf.velocities.u.parent(), "v": vbar.parent(), "c0": bgf.tracers.b.parent()}
    yard = B.BackgroundOrchestrated(oracle, g_cpu, 2, NU, (KAPPA["b"], KAPPA["S"]), background=background, buoyancy_index=0, fcor=FCOR,
                                    forcing={"c1": forcing} if forced else None, closure="numpy",
                                    bcs={"c0": {"top": ("value", 0.4)}, "c1": {"bottom": ("flux", 0.03)}})
    nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
    vals = smooth_state({("T" if n == "b" else n): v for n, v in nodes.items()}, 17)
    vals["b"] = vals.pop("T")
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["b"], c1=vals["S"])
    return grid, model, yard, background


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "substep_in_epilogue"])
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("name", list(MODEL_GRIDS))
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, name, timestepper, forced):
    """2 steps with backgrounds on u (function), v (Field) and b (non-periodic along the Periodic x) but not on S, ScalarDiffusivity,
    BuoyancyTracer, FPlane, an array forcing on S, a Value condition on b's top and a Flux condition on S's bottom: u, v, w, b, S to
    1e-12, p on the scale of test_gpu_vertically_implicit.test_model_is_the_orchestrated_yardstick, the clock `==`. Without the forcing
    the RK3 substep of stages 2 and 3 rides in the epilogue pass behind both advection terms."""
    grid, model, yard, background = _model_pair(ocn, oracle, arch, name, timestepper, forced)
    assert model.get_option("background_fields") == 3
    assert model.get_option("background_tendency_path") == (2 if name == "ppb_stretched" else 1)
    # the substep of stages 2 and 3 rides in the epilogue pass, which closes the cells after both advection terms -- but not with a forcing
    assert model.get_option("fuse_substep_active") == (0 if forced else 1) and model.get_option("substep_in_tendency_kernel") == 0
    # the function's halo along the Periodic x is its analytic continuation
    b_bg = background["c0"]
    assert b_bg[0, 5, 5] < b_bg[3, 5, 5] < b_bg[-1, 5, 5] and b_bg[0, 5, 5] != b_bg[grid.Nx, 5, 5]
    dt = 0.05 / grid.Nx
    for _ in range(2):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    core = (slice(3, -3),) * 3
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    for gn, cn in zip(("u", "v", "w", "b", "S"), yard.names):
        a, b = model.fields()[gn].parent()[core], yard.U[cn][core]
        assert np.all(np.isfinite(a))
        print(f"{name} {timestepper} {gn}: rel_err {rel_err(a, b):.3e}")
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = model.pressures.pNHS.parent()[core], yard.p[core]
    pscale = max(np.abs(b).max(), umax * max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / dt)
    print(f"{name} {timestepper} p: max abs difference {np.max(np.abs(a - b)):.3e} on the scale {pscale:.3e}")
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == 2
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    # the totals the last update_state! left: the model's own u, v plus the backgrounds, halos included
    for n in "uv":
        assert np.array_equal(model._field("total_" + n).parent(), model.fields()[n].parent() + background[n])
    model.close()


def _plain_pair(ocn, arch, size, background_fields, **kw):
    out = []
    for bg in (None, background_fields):
        grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), background_fields=bg(grid) if bg else None, **kw)
        vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 9)
        ocn.set_model(model, **vals)
        out.append(model)
    return out


def test_all_zero_backgrounds_change_nothing(ocn, arch):
    """explicit all-zero arrays for every field (both terms and the totals are evaluated, the substep leaves the tendency launch): after 2
    RK3 steps on PPP (16, 16, 16) every field equals the model built without backgrounds"""
    def zeros(grid):
        return {n: np.zeros(grid.total_size(loc)) for n, loc in
                (("u", (ocn.Face, ocn.Center, ocn.Center)), ("v", (ocn.Center, ocn.Face, ocn.Center)), ("w", (ocn.Center, ocn.Center, ocn.Face)),
                 ("T", (ocn.Center,) * 3), ("S", (ocn.Center,) * 3))}
    plain, bg = _plain_pair(ocn, arch, (16, 16, 16), zeros)
    assert bg.get_option("background_fields") == 5 and bg.get_option("background_tendency_path") == 2 and plain.get_option("background_fields") == 0
    assert plain.get_option("background_tendency_path") == 0 and plain.get_option("fuse_substep_active") == 1
    for _ in range(2):
        ocn.time_step(plain, 0.004)
        ocn.time_step(bg, 0.004)
    for n in plain.fields():
        a, b = bg.fields()[n].parent(), plain.fields()[n].parent()
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (n, np.abs(a - b).max())
    assert np.array_equal(bg.pressures.pNHS.parent(), plain.pressures.pNHS.parent())
    plain.close()
    bg.close()


def test_cell_advection_timescale_and_wizard_see_the_totals(ocn, oracle, arch):
    size = (16, 16, 12)
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(12), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    g_cpu = oracle.Grid(size, topology=(0, 0, 1), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(12))
    bgs = {"u": 3.0, "v": lambda x, y, z: np.sin(2 * np.pi * x) + 0 * y + 0 * z, "w": lambda x, y, z: 0.5 * z * (z + 1) + 0 * x + 0 * y}
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), background_fields=bgs)
    plain = ocn.NonhydrostaticModel(grid=grid, tracers=("T",))
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 3)
    ocn.set_model(model, **vals)
    ocn.set_model(plain, **vals)
    L = oracle.lib()
    import ctypes as C
    L.oro_cell_advection_timescale.restype = C.c_double
    L.oro_cell_advection_timescale.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
    tot = [np.asfortranarray(model.fields()[n].parent() + getattr(model.background_fields.velocities, n).parent()) for n in "uvw"]
    want = L.oro_cell_advection_timescale(g_cpu.handle, *[oracle._dp(a) for a in tot])
    got = ocn.cell_advection_timescale(model)
    print(f"cell_advection_timescale: library {got!r} oracle {want!r} without backgrounds {ocn.cell_advection_timescale(plain)!r}")
    assert got == want
    assert got < 0.5 * ocn.cell_advection_timescale(plain)            # Ū = 3 dominates: the model's own velocities alone give a much longer one
    wizard = ocn.TimeStepWizard(cfl=0.5, max_change=1e9, min_change=1e-9)
    sim = type("S", (), {})()
    sim.model, sim.Δt = model, 1.0
    wizard(sim)
    assert sim.Δt == 0.5 * want
    model.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# the reference's data-free arms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_internal_wave_with_background_stratification(ocn, arch, timestepper):
    """"Background fields" of test_dynamics.jl:713-730: internal_wave_solution(background_stratification = true) -- b carries the wave
    only, the stratification N² z is background_fields.b -- on 128 x 4 x 128 (Ny = 4 instead of 1: the adaptation of the explicit twin,
    tests/test_gpu_reference_tests.py::test_internal_wave_dynamics); 10 steps; relative_error(u) < 1e-4 and the wave did propagate"""
    Lx, Nx, Nz = 2 * np.pi, 128, 128
    grid = ocn.RectilinearGrid(arch, size=(Nx, 4, Nz), x=(0.0, Lx), y=(0.0, Lx), z=(-Lx, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    f, NN, mz, kx, a0 = 0.2, 1.0, 16, 1, 1e-3
    z0, d = -Lx / 3, Lx / 20
    sig = np.sqrt((NN ** 2 * kx ** 2 + f ** 2 * mz ** 2) / (kx ** 2 + mz ** 2))
    dt = 0.01 / sig
    cg = mz * sig / (kx ** 2 + mz ** 2) * (f ** 2 / sig ** 2 - 1)
    U, V = a0 * kx * sig / (sig ** 2 - f ** 2), a0 * kx * f / (sig ** 2 - f ** 2)
    W, Bw = a0 * mz * sig / (sig ** 2 - NN ** 2), a0 * mz * NN ** 2 / (sig ** 2 - NN ** 2)

    def a(zz, t):
        return np.exp(-(zz - cg * t - z0) ** 2 / (2 * d) ** 2)

    def u(x, y, zz, t=0.0):
        return a(zz, t) * U * np.cos(kx * x + mz * zz - sig * t) + 0 * y
    model = ocn.NonhydrostaticModel(grid=grid, closure=ocn.ScalarDiffusivity(ν=1e-9, κ=1e-9), buoyancy=ocn.BuoyancyTracer(), tracers=("b",),
                                    coriolis=ocn.FPlane(f=f), timestepper=timestepper,
                                    background_fields={"b": lambda x, y, zz, t: NN ** 2 * zz + 0 * (x + y)})
    assert model.get_option("background_fields") == 1 and model.get_option("background_tendency_path") == 2
    ocn.set_model(model, u=u, v=lambda x, y, zz: a(zz, 0) * V * np.sin(kx * x + mz * zz) + 0 * y,
                  w=lambda x, y, zz: a(zz, 0) * W * np.cos(kx * x + mz * zz) + 0 * y,
                  b=lambda x, y, zz: a(zz, 0) * Bw * np.sin(kx * x + mz * zz) + 0 * y)
    for _ in range(10):
        ocn.time_step(model, dt)
    uf = model.fields()["u"]
    x, y, zz = grid.nodes(uf.loc)
    exact = u(x, y, zz, model.clock.time)
    got = uf.interior()
    print(f"internal wave {timestepper}: relative_error(u) {np.mean((got - exact) ** 2) / np.mean(exact ** 2):.3e}, against the initial u "
          f"{np.mean((got - u(x, y, zz, 0.0)) ** 2) / np.mean(exact ** 2):.3e}")
    assert np.mean((got - exact) ** 2) / np.mean(exact ** 2) < 1e-4
    assert np.mean((got - u(x, y, zz, 0.0)) ** 2) / np.mean(exact ** 2) > 1e-4          # the wave did propagate
    model.close()


def test_time_stepping_with_background_fields(ocn, arch):
    """time_stepping_with_background_fields (test_time_stepping.jl:201-240) on 4 x 4 x 4 instead of 1 x 1 x 1, the exp(t) factor of
    background_v dropped (time-independent backgrounds only): the locations of all six backgrounds and one finite time-step. The
    reference's ConstantField R has no location; here it is a ccc array full of the number."""
    grid = ocn.RectilinearGrid(arch, size=(4, 4, 4), extent=(1, 1, 1))
    p = dict(α=1.2, β=0.2, λ=43)
    background_u = lambda x, y, z, t: np.pi + 0 * (x + y + z)                               # noqa: E731
    bgs = dict(u=background_u, v=lambda x, y, z, t: np.sin(x) * np.cos(y) + 0 * z,
               w=ocn.BackgroundField(lambda x, y, z, t, q: q["α"] * x + q["β"] * np.exp(z / q["λ"]) + 0 * y, parameters=p),
               T=background_u, S=ocn.BackgroundField(lambda x, y, z, t, α: α * y + 0 * (x + z), parameters=1.2), R=ocn.BackgroundField(1))
    model = ocn.NonhydrostaticModel(grid=grid, background_fields=bgs, buoyancy=ocn.SeawaterBuoyancy(), tracers=("T", "S", "R"))
    ocn.time_step(model, 1)
    F, Cn = ocn.Face, ocn.Center
    bf = model.background_fields
    assert bf.velocities.u.loc == (F, Cn, Cn) and bf.velocities.v.loc == (Cn, F, Cn) and bf.velocities.w.loc == (Cn, Cn, F)
    assert bf.tracers.T.loc == bf.tracers.S.loc == bf.tracers.R.loc == (Cn, Cn, Cn)
    assert np.all(bf.tracers.R.parent() == 1.0) and np.all(bf.tracers.T.parent() == np.pi)
    assert model.get_option("background_fields") == 6
    for n, fld in model.fields().items():
        assert np.all(np.isfinite(fld.parent())), n
    assert model.clock.iteration == 1 and model.clock.time == 1.0
    model.close()


def test_captured_step_matches_the_uncaptured_one(ocn, arch):
    """a background model steps with the default `use_graph` option: the total-velocity buffers exist before the capture (the setter made
    them), the step is captured once and replayed, and the fields equal those of the same model stepped with the graph off"""
    def bgs(grid):
        return {"u": lambda x, y, z: 0.3 * np.sin(2 * np.pi * z) + 0 * x + 0 * y, "T": lambda x, y, z: 2.0 * z + 0.5 * x + 0 * y}
    models = []
    for use_graph in (1, 0):
        grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), extent=(1, 1, 1))
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), background_fields=bgs(grid))
        model.set_option("use_graph", use_graph)
        vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 9)
        ocn.set_model(model, **vals)
        for _ in range(4):
            ocn.time_step(model, 0.004)
        models.append(model)
    g, plain = models
    assert g.get_option("use_graph") == 1 and g.get_option("graph_captures") == 1 and g.get_option("graph_replays") >= 1
    assert g.get_option("graph_failures") == 0 and plain.get_option("graph_captures") == 0
    for n in g.fields():
        assert np.array_equal(g.fields()[n].parent(), plain.fields()[n].parent()), n
    assert np.array_equal(g._field("total_u").parent(), plain._field("total_u").parent())
    assert g.clock.time == plain.clock.time
    for m in models:
        m.close()
