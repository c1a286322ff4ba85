"""ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) on the MI355X against the numpy restatement
(tests/vertically_implicit_reference.py, pinned on the CPU by tests/test_vertically_implicit_host.py):
  * the tridiagonal solve along z bit for bit, halos untouched;
  * the explicit part through the raw entry point, bit for bit;
  * the model (RK3 and AB2, the substep riding in the tendency launch and on its own) against the orchestrated yardstick, 1e-12;
  * the x-slab partition inside the library against the single-GPU model;
  * the vertically implicit arms of the reference's data-free diffusion tests (test/test_dynamics.jl:404-458,536-542);
  * a column stepped at 50 times the explicit diffusive limit."""
import ctypes as C

import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import vertically_implicit_reference as R

pytestmark = pytest.mark.gpu

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))

# (70, 5, 13): two waves with a ragged tail in x, Nz no multiple of the batch of levels; (12, 10, 8) BBB: wall-face columns of u and v;
# Nz = 2: the loops degenerate; a column; a (Periodic, Flat, Bounded) slice
GRIDS = {
    "ppb_stretched": dict(size=(70, 5, 13), topo="PPB", stretched=True),
    "bbb": dict(size=(12, 10, 8), topo="BBB", stretched=False),
    "nz2": dict(size=(9, 4, 2), topo="PPB", stretched=True),
    "column": dict(size=(16,), topo="FFB", stretched=False),
    "slice": dict(size=(66, 16), topo="PFB", stretched=False),
}


def _grid(ocn, arch, name):
    c = GRIDS[name]
    topo = tuple({"P": ocn.Periodic, "B": ocn.Bounded, "F": ocn.Flat}[t] for t in c["topo"])
    Nz = c["size"][-1]
    kw = dict(z=tanh_faces(Nz) if c["stretched"] else (-1.0, 0.0))
    if topo[0] is not ocn.Flat:
        kw["x"] = (0.0, 1.0)
    if topo[1] is not ocn.Flat:
        kw["y"] = (0.0, 1.0)
    return ocn.RectilinearGrid(arch, size=c["size"], topology=topo, **kw)


def _random_fields(ocn, grid, seed):
    """u, v, w, c with random values in the WHOLE parent array (halos included) -> (dict name -> Field, dict name -> parent array)"""
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}
    flds, parents = {}, {}
    for n in "uvwc":
        f = make[n](grid)
        a = np.asfortranarray(rng.standard_normal(f.shape))
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


@pytest.mark.parametrize("name", list(GRIDS))
def test_solve_kernel_is_the_restatement_bit_for_bit(ocn, arch, name):
    """the solve == the numpy Thomas sweep on random u, v, w and tracer fields, off-diagonals O(1) and O(100); the parent
    array outside the solved columns and levels keeps its bits"""
    grid = _grid(ocn, arch, name)
    m = R.Metrics.of_grid(grid)
    coef = 1.7
    for r in (1.0, 100.0):
        dt = r * float(m.dzc[m.H[2]:m.H[2] + m.N[2]].min()) ** 2 / coef
        flds, parents = _random_fields(ocn, grid, 21)
        for n in "uvwc":
            before = parents[n]
            want = R.implicit_step(m, before.copy(order="F"), R.LOCS[n], coef, dt)
            assert not np.array_equal(want, before)
            for form in (0,):           # the forms shipped: the reference-shaped kernel alone (the tuned ones measured slower)
                flds[n].set_parent(before)
                ocn.kernels.implicit_step(grid, flds[n], coef, dt, form=form)
                got = flds[n].parent()
                assert np.array_equal(got, want), (n, r, form, np.abs(got - want).max())
                solved = np.zeros(got.shape, dtype=bool)
                solved[m.H[0]:m.H[0] + m.N[0], m.H[1]:m.H[1] + m.N[1], m.H[2]:m.H[2] + m.N[2]] = True
                assert np.array_equal(got[~solved], before[~solved]), (n, r, form)


def test_solve_entry_point_refusals(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    grid = ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1))
    f = ocn.CenterField(grid)
    with pytest.raises(ocn.OcnError, match="Bounded in the z-direction"):
        ocn.kernels.implicit_step(grid, f, 1.0, 0.1)
    grid = _grid(ocn, arch, "bbb")
    f = ocn.CenterField(grid)
    with pytest.raises(ocn.OcnError, match="form"):
        ocn.kernels.implicit_step(grid, f, 1.0, 0.1, form=1)
    assert _lib.lib().ocn_implicit_step_z(grid.handle, f.data, _lib.i3((1, 1, 0)), 1.0, 0.1, 0) != 0
    # the model setter: Periodic z is the reference's error; an eddy-coefficient closure clears the setting
    model = ocn.NonhydrostaticModel(grid=ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1)))
    assert _lib.lib().ocn_model_set_vertically_implicit(model.handle, 1) == -1
    assert b"Bounded in the z-direction" in _lib.lib().ocn_last_error()
    model = ocn.NonhydrostaticModel(grid=grid, closure=ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=1e-3))
    assert model.get_option("vertically_implicit") == 1 and model.get_option("epilogue_march_active") == 0
    kappa = (C.c_double * 2)(1 / 3, 1 / 3)
    _lib.check(_lib.lib().ocn_model_set_amd(model.handle, 1 / 3, kappa))
    assert model.get_option("vertically_implicit") == 0
    assert _lib.lib().ocn_model_set_vertically_implicit(model.handle, 1) != 0


@pytest.mark.parametrize("name", list(GRIDS))
def test_explicit_part_is_the_restatement_bit_for_bit(ocn, arch, name):
    grid = _grid(ocn, arch, name)
    m = R.Metrics.of_grid(grid)
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=0.37, κ=0.11)
    flds, P = _random_fields(ocn, grid, 31)
    ranges = [None]
    if name == "ppb_stretched":
        ranges.append((3, 68, 2, 4, 1, 13))             # a launch range: both z-flux boundary indices inside, x and y trimmed
    for rng in ranges:
        G, G0 = _random_fields(ocn, grid, 32)
        ocn.kernels.compute_closure_tendencies_vertically_implicit(grid, [flds[n] for n in "uvwc"], [G[n] for n in "uvwc"], closure, ("c",),
                                                                   kernel_parameters=rng)
        for n in "uvwc":
            coef = closure.ν if n != "c" else closure.κ
            want = R.explicit_part(m, n, P, P["c"], coef, G0[n].copy(order="F"), vi=True, rng=rng)
            got = G[n].parent()
            assert np.array_equal(got, want), (n, rng, np.abs(got - want).max())
            assert not np.array_equal(got, G0[n])
            explicit = R.explicit_part(m, n, P, P["c"], coef, G0[n].copy(order="F"), vi=False, rng=rng)
            assert not np.array_equal(got, explicit)


# ---------------------------------------------------------------------------------------------------------------------
# the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA = 2e-3, {"T": 5e-3, "S": 1e-3}
MODEL_GRIDS = {"ppb_stretched": ((16, 16, 12), ("Periodic", "Periodic", "Bounded"), True), "bbb": ((12, 10, 8), ("Bounded",) * 3, False)}


def _model_pair(ocn, oracle, arch, name, timestepper):
    size, topology, stretched = MODEL_GRIDS[name]
    z = tanh_faces(size[2]) if stretched else (-1.0, 0.0)
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=tuple(getattr(ocn, t) for t in topology))
    g_cpu = oracle.Grid(size, topology=tuple(int(t == "Bounded") for t in topology), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    F = ocn.FieldBoundaryConditions
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), timestepper=timestepper,
                                    closure=ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=NU, κ=KAPPA),
                                    boundary_conditions={"T": F(top=ocn.ValueBoundaryCondition(0.4)), "S": F(bottom=ocn.FluxBoundaryCondition(0.03))})
    yard = R.Orchestrated(oracle, g_cpu, 2, NU, (KAPPA["T"], KAPPA["S"]), closure="vi",
                          bcs={"c0": {"top": ("value", 0.4)}, "c1": {"bottom": ("flux", 0.03)}})
    vals = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 17)
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["T"], c1=vals["S"])
    return grid, model, yard


@pytest.mark.parametrize("timestepper,fuse", [("RungeKutta3", 1), ("RungeKutta3", 0), ("QuasiAdamsBashforth2", 1)],
                         ids=["rk3_substep_in_tendency_launch", "rk3_substep_on_its_own", "ab2"])
@pytest.mark.parametrize("name", list(MODEL_GRIDS))
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, name, timestepper, fuse):
    """2 steps with ν ≠ κ_T ≠ κ_S, a Value condition on T's top (the boundary-face rule) and a Flux condition on S's bottom: u, v, w, T, S
    to 1e-12, p against the scale of test_gpu_parity.test_time_step_parity_10_steps, the clock `==`"""
    grid, model, yard = _model_pair(ocn, oracle, arch, name, timestepper)
    model.set_option("fuse_substep", fuse)
    assert model.get_option("vertically_implicit") == 1 and model.get_option("epilogue_march_active") == 0
    assert model.get_option("fuse_substep_active") == fuse          # the stages 2 and 3 substep rides in the tendency launch, or runs alone
    dt = 0.05 / grid.Nx
    for _ in range(2):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    core = (slice(3, -3),) * 3
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    for gn, cn in zip(("u", "v", "w", "T", "S"), yard.names):
        a, b = model.fields()[gn].parent()[core], yard.U[cn][core]
        assert np.all(np.isfinite(a))
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = model.pressures.pNHS.parent()[core], yard.p[core]
    pscale = max(np.abs(b).max(), umax * max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / dt)
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == 2
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    model.close()


@pytest.mark.parametrize("xbounded", [False, True], ids=["ppb", "bounded_x"])
def test_partitioned_model_matches_the_single_gpu_model(ocn, arch, monkeypatch, xbounded):
    """two x-slabs inside the library on virtual ranks (tests/test_gpu_dist_library.py's helpers, its "bounded" preset with the closure
    made vertically implicit): z is never partitioned, so the solve runs per slab; on a Bounded partitioned x only the end ranks own a
    wall column of u. Against the single-GPU vertically implicit model -- which the test above holds to the yardstick -- 1e-12."""
    import test_gpu_dist_library as D
    base = D._closure

    def implicit(ocn_, zkind):
        c = base(ocn_, zkind)
        return ocn_.ScalarDiffusivity(ocn_.VerticallyImplicitTimeDiscretization(), ν=c.ν, κ=c.κ)
    monkeypatch.setattr(D, "_closure", implicit)
    D._own_stream()
    R_, size, nsteps = 2, (32, 12, 10), 2
    seen = []
    results = D._run_library_ranks(ocn, arch, R_, size, nsteps, "bounded", {}, xbounded=xbounded,
                                   probe=lambda model: seen.append(model.get_option("vertically_implicit")))
    ref, time, _ = D._single_gpu(ocn, arch, size, "bounded", nsteps, xbounded=xbounded)
    assert seen == [1, 1]
    for r, (out, div, t, _off) in enumerate(results):
        assert div < 5e-8 and t == time
        D._compare(out, ref, r, size[0] // R_, size)


# ---------------------------------------------------------------------------------------------------------------------
# the vertically implicit arms of the reference's data-free tests (their explicit twins: tests/test_gpu_reference_tests.py)
# ---------------------------------------------------------------------------------------------------------------------
def _vi(ocn, **kw):
    return ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), **kw)


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_diffusion_simple(ocn, arch, timestepper):
    """test_diffusion_simple (test_dynamics.jl:17-32,404-411) with VerticallyImplicitTimeDiscretization: a field equal to π stays π over
    10 steps of Δt = 1 (one-cell x, y made Flat as in the explicit twin)"""
    for name in ("u", "v", "c"):
        grid = ocn.RectilinearGrid(arch, size=(16,), z=(-1.0, 0.0), topology=(ocn.Flat, ocn.Flat, ocn.Bounded))
        model = ocn.NonhydrostaticModel(grid=grid, closure=_vi(ocn, ν=1.0, κ=1.0), timestepper=timestepper, tracers=("c",))
        f = model.fields()[name]
        f.set(np.pi)
        ocn.update_state(model)
        for _ in range(10):
            ocn.time_step(model, 1.0)
        assert np.allclose(f.interior(), np.pi, rtol=SQRT_EPS, atol=0), name
        model.close()


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("topology", [("Periodic", "Periodic", "Bounded"), ("Periodic", "Bounded", "Bounded"), ("Bounded", "Bounded", "Bounded")])
def test_scalar_diffusivity_budget(ocn, arch, topology, timestepper):
    """test_ScalarDiffusivity_budget (test_dynamics.jl:34-56,413-461), the vertically implicit arm (not on a Periodic z, :421-426): the
    mean of c, and of u / v where their direction is Periodic (w is left out on a Bounded z, :436-439), is kept"""
    names = ["c"] + [n for n, t in zip("uvw", topology) if t == "Periodic"]
    rng = np.random.default_rng(5)
    for name in names:
        grid = ocn.RectilinearGrid(arch, size=(4, 4, 4), extent=(1, 1, 1), topology=tuple(getattr(ocn, t) for t in topology))
        model = ocn.NonhydrostaticModel(grid=grid, closure=_vi(ocn, ν=1.0, κ=1.0), timestepper=timestepper, tracers=("c",))
        ocn.set_model(model, u=0.0, v=0.0, w=0.0, c=0.0)
        ocn.set_model(model, **{name: lambda x, y, z: rng.random(np.broadcast(x, y, z).shape)})
        f = model.fields()[name]
        before = f.interior().mean()
        ocn.update_state(model)
        for _ in range(10):
            ocn.time_step(model, 1e-4 * 0.25 ** 2)
        after = f.interior().mean()
        assert abs(after - before) <= SQRT_EPS * max(abs(after), abs(before)), (name, before, after)
        model.close()


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_diffusion_cosine(ocn, arch, timestepper):
    """test_diffusion_cosine (test_dynamics.jl:65-87) with ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν = κ = 1) on the grid
    of the explicit twin ((4, 4, 128), z in (0, π/2)): cos(2 z) in u, v or c decays as exp(-4 t), isapprox(atol = rtol = 1e-6)"""
    N, Lz = 128, np.pi / 2
    for name in ("u", "v", "c"):
        grid = ocn.RectilinearGrid(arch, size=(4, 4, N), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, Lz),
                                   topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        model = ocn.NonhydrostaticModel(grid=grid, closure=_vi(ocn, ν=1.0, κ=1.0), timestepper=timestepper, tracers=("c",))
        f = model.fields()[name]
        x, y, z = grid.nodes(f.loc)
        f0 = np.cos(2 * z) + 0 * (x + y)
        f.set(f0)
        ocn.update_state(model)
        for _ in range(5):
            ocn.time_step(model, 1e-6 * Lz ** 2)
        exact = np.exp(-4 * model.clock.time) * f0
        got = f.interior()
        assert np.linalg.norm(got - exact) <= max(1e-6, 1e-6 * max(np.linalg.norm(got), np.linalg.norm(exact))), name
        model.close()


def test_a_column_steps_at_fifty_times_the_explicit_limit(ocn, arch):
    """what the feature is for: a (Flat, Flat, Bounded) column, Nz = 64 stretched, κ = 1, c = cos(2 z), 5 RK3 steps of Δt = 50 Δz_min² / κ:
    no NaN, max |c| never increases, and the result is the dense numpy solution of the same stage chain. With u = v = w = 0 and no x, y
    extent the explicit part of a stage is the boundary-face flux only -- zero, the default no-flux condition -- so a stage is
    c <- (1 - Δt_stage ∂z κ ∂z)⁻¹ c; the tolerance is the dense-solve bound of tests/test_vertically_implicit_host.py, summed over the
    15 solves (the max norm of every stage operator's inverse is <= 1: diagonal >= 1, non-positive off-diagonals)."""
    from test_vertically_implicit_host import dense_tolerance
    Nz = 64
    grid = ocn.RectilinearGrid(arch, size=(Nz,), z=tanh_faces(Nz, Lz=np.pi / 2), topology=(ocn.Flat, ocn.Flat, ocn.Bounded))
    model = ocn.NonhydrostaticModel(grid=grid, closure=_vi(ocn, ν=1.0, κ=1.0), tracers=("c",))
    c = model.tracers.c
    z = grid.nodes(c.loc)[2]
    c0 = np.cos(2 * z).reshape(1, 1, Nz)
    ocn.set_model(model, c=c0)
    m = R.Metrics.of_grid(grid)
    dt = 50 * float(m.dzc[m.H[2]:m.H[2] + Nz].min()) ** 2 / 1.0
    dense, tol, peak = c0.reshape(Nz).copy(), 0.0, np.abs(c0).max()
    for _ in range(5):
        ocn.time_step(model, dt)
        got = c.interior()
        assert np.all(np.isfinite(got))
        assert np.abs(got).max() <= peak
        peak = np.abs(got).max()
        for sdt in (dt * R.G1, dt * (R.G2 + R.Z2), dt * (R.G3 + R.Z3)):
            a, b, cc = R.diagonals(m, R.LOCS["c"], 1.0, sdt)
            A = R.dense_matrix(a, b, cc, 0, 0)
            dense = np.linalg.solve(A, dense)
            tol += dense_tolerance(A, dense)
    assert np.abs(c.interior().reshape(Nz) - dense).max() <= tol, (np.abs(c.interior().reshape(Nz) - dense).max(), tol)
    # and it did diffuse: mode 2 decays as exp(-4 t); backward Euler stages decay it more slowly, by at least half as much at 4 Δt << 1
    t = model.clock.time
    assert 4 * t < 0.2 and 1 - np.abs(dense).max() / np.abs(c0).max() >= 0.5 * (1 - np.exp(-4 * t))
    model.close()
