"""GPU tests of the forcing term (ocn_forcing.h, ocn_model_set_forcing; reference src/Forcings/ and the last term of
nonhydrostatic_tendency_kernel_functions.jl:81-93).

  * tendency identity, bitwise: after update_state!, G of a forced model == G of the same model without forcing + F, F evaluated in
    numpy from the same tables and arrays (forcings.evaluate), on the role-kernel, per-value epilogue (FPlane), marching epilogue
    (ScalarDiffusivity) and per-field kernel ((Bounded, Periodic, Bounded)) configurations, and with the standalone pass forced; the
    first and the last of these also at sizes of several 64 x 7 tiles of the role kernel;
  * the two forcing-path options give `==` fields after RK3 steps, also across tile seams;
  * known answers: T ≡ 1 relaxed to 0 at rate 1/τ follows the RK3 stability polynomial / the AB2 recurrence;
  * test/test_forcings.jl's relaxed_time_stepping, two_forcings and seven_forcings, adapted to closure-free forcings;
  * a borrowed Field forcing acts with the value it has when the tendency is evaluated;
  * x-slab partitions (R = 2, 4) against the single-GPU model."""
import threading

import numpy as np
import pytest

from helpers import smooth_state, tanh_faces

pytestmark = pytest.mark.gpu


def _locs(ocn):
    return {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face)}


def _kernel_range(grid, loc, ocn, velocity):
    """the interior range the tendency launch covers: the first Face index of a Bounded direction is excluded for velocities"""
    out = []
    for d, (n, l, t) in enumerate(zip(grid.interior_size(loc), loc, grid.topology)):
        lo = 1 if (velocity and l is ocn.Face and t is ocn.Bounded and grid.size[d] > 1) else 0
        hi = grid.size[d]
        out.append(slice(lo, hi))
    return tuple(out)


def _state(ocn, grid, model, seed=3):
    nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
    return smooth_state(nodes, seed)


def _pair(ocn, arch, grid_kw, forcing, options=None, **model_kw):
    models = []
    for frc in (None, forcing):
        grid = ocn.RectilinearGrid(arch, **grid_kw)
        m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), forcing=frc, **model_kw)
        for k, v in (options or {}).items():
            m.set_option(k, v)
        models.append(m)
    vals = _state(ocn, models[0].grid, models[0])
    for m in models:
        ocn.set_model(m, **vals)
        ocn.update_state(m)
    return models


def _check_identity(ocn, plain, forced):
    from oldoceananigans_jl_amd import forcings as F
    grid = forced.grid
    for name, fld in forced.fields().items():
        G0 = plain.tendency(name).interior()
        G1 = forced.tendency(name).interior()
        terms = forced._forcing_terms.get(name)
        if not terms:
            assert np.array_equal(G0, G1), name
            continue
        phi = fld.interior()
        want = G0.copy()
        r = _kernel_range(grid, fld.loc, ocn, name in ("u", "v", "w"))
        want[r] = G0[r] + F.evaluate(terms, grid, fld.loc, phi)[r]
        assert np.array_equal(G1, want), (name, np.abs(G1 - want).max())


def _sponge(ocn, D, center, width, rate=0.7, target=None):
    return ocn.Relaxation(rate=rate, mask=ocn.GaussianMask(D, center=center, width=width),
                          target=target if target is not None else ocn.LinearTarget(D, intercept=0.3, gradient=0.2))


def _forcing_set(ocn, size, rng):
    """masks along x, y and z; zero, constant and linear targets; an array; 2- and 5-term sums"""
    arr = rng.standard_normal(size)
    return {
        "u": _sponge(ocn, "x", 0.5, 0.2),
        "v": (ocn.Relaxation(rate=0.4, mask=ocn.PiecewiseLinearMask("y", center=0.5, width=0.3), target=1.5), ocn.Relaxation(rate=0.1)),
        "w": ocn.Relaxation(rate=0.9, mask=ocn.GaussianMask("z", center=-0.5, width=0.25)),
        "T": ocn.MultipleForcings(_sponge(ocn, "z", -0.2, 0.3), ocn.Forcing(arr), ocn.Relaxation(rate=0.05, target=2.0),
                                  _sponge(ocn, "x", 0.1, 0.4), ocn.Relaxation(rate=0.2, mask=ocn.PiecewiseLinearMask("x", center=0.7, width=0.5))),
        "S": 0.5 * arr,
    }


# (name, topology, physics, options, expected "forcing_path"): 1 = inside the role tendency kernel, 3 = the standalone pass after the
# tendency launch(es) -- physics epilogue (per-value with FPlane, marching with ScalarDiffusivity), per-field kernels (Bounded x), Bounded z
CASES = [
    ("role kernel", "PPP", {}, {}, 1),
    ("standalone, forced by option", "PPP", {}, {"fused_forcing": 0}, 3),
    ("role kernel, Bounded z", "PPB", {}, {}, 3),
    ("per-value epilogue", "PPB", {"coriolis": True}, {}, 3),
    ("marching epilogue", "PPB", {"closure": True}, {}, 3),
    ("per-field kernels", "BPB", {}, {}, 3),
    ("with a top Flux condition", "PPB", {"flux": True}, {}, 3),
]


# Sizes around the 64 x 7 tiles of the role kernel (those of test_gpu_parity.test_tile_edges_of_the_tendency_kernels that a second x tile,
# a row tile ending on the range's last row or a live edge wave need): in a second tile the FORCE branch's clamped index
# (min(i, i1), min(j, j1), max(k - 1, k0)) and the tables of a Relaxation, indexed i - 1 + Hx, start at i0 = 65, 129.
TILE_SIZES = [(65, 8, 6), (129, 15, 5), (64, 7, 7), (130, 6, 9)]


def _identity(ocn, arch, case, size):
    _, topology, physics, options, path = case
    topo = tuple(ocn.Periodic if t == "P" else ocn.Bounded for t in topology)
    z = tanh_faces(size[2]) if topology[2] == "B" else (-1.0, 0.0)
    kw = dict(size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=topo)
    model_kw = {}
    if physics.get("coriolis"):
        model_kw["coriolis"] = ocn.FPlane(f=0.7)
    if physics.get("closure"):
        model_kw["closure"] = ocn.ScalarDiffusivity(ν=1e-3, κ=2e-3)
    if physics.get("flux"):
        model_kw["boundary_conditions"] = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-2))}
    rng = np.random.default_rng(11)
    plain, forced = _pair(ocn, arch, kw, _forcing_set(ocn, size, rng), options, **model_kw)
    assert plain.get_option("forcing_path") == 0
    assert forced.get_option("forcing_path") == path
    # the role-kernel path keeps the RK3 substep riding in the tendency launch; the standalone pass runs it separately
    assert forced.get_option("fuse_substep_active") == plain.get_option("fuse_substep_active") * (path == 1)
    _check_identity(ocn, plain, forced)
    return forced


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tendency_identity_bitwise(ocn, arch, case):
    _identity(ocn, arch, case, (16, 12, 10))


@pytest.mark.parametrize("size", TILE_SIZES, ids=["x".join(map(str, s)) for s in TILE_SIZES])
@pytest.mark.parametrize("case", CASES[:2], ids=[c[0] for c in CASES[:2]])
def test_tendency_identity_bitwise_across_tile_edges(ocn, arch, case, size):
    """the identity in and after a role kernel of several tiles: forcing_sum of the in-kernel path evaluates cells of a second and third
    x tile, of a row tile whose last row is the range's, and beside a live edge-wave column; the x masks of _forcing_set (Gaussians at 0.5
    and 0.1, piecewise linear at 0.7) differ from column 64 to column 65, so a table read one tile or one column off is seen"""
    forced = _identity(ocn, arch, case, size)
    Hx = forced.grid.halo_size[0]
    tables = [t.mask_table for terms in forced._forcing_terms.values() for t in terms if t.kind == 2 and t.mask_dir == 0]
    assert len(tables) == 3
    for table in tables:
        assert table[64 - 1 + Hx] != table[65 - 1 + Hx] and table[64 - 1 + Hx] != 0.0


def _fused_and_standalone_steps(ocn, arch, size, substep_rides=False):
    fields = []
    for fused in (1, 0):
        grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
        m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), forcing=_forcing_set(ocn, size, np.random.default_rng(5)))
        m.set_option("fused_forcing", fused)
        assert m.get_option("forcing_path") == (1 if fused else 3)
        assert not substep_rides or m.get_option("fuse_substep_active") == fused
        ocn.set_model(m, **_state(ocn, grid, m))
        for _ in range(3):
            ocn.time_step(m, min(0.01, 0.1 * grid.Δxᶜᵃᵃ / 0.6))
        fields.append({n: f.parent() for n, f in m.fields().items()})
    for n in fields[0]:
        assert np.array_equal(fields[0][n], fields[1][n]), n
        assert np.all(np.isfinite(fields[0][n])) and np.abs(fields[0][n]).max() > 0


def test_role_kernel_and_standalone_forcing_agree_over_rk3_steps(ocn, arch):
    """forcing inside the role kernel with the fused RK3 substep (path 1) == the standalone pass with separate substeps (path 3)"""
    _fused_and_standalone_steps(ocn, arch, (16, 16, 16))


@pytest.mark.parametrize("size", TILE_SIZES[:2], ids=["x".join(map(str, s)) for s in TILE_SIZES[:2]])
def test_role_kernel_and_standalone_forcing_agree_across_tile_edges(ocn, arch, size):
    """the same 3 RK3 steps at 65 x 8 x 6 and 129 x 15 x 5: the forcing term together with the substep that rides in the kernel, across
    the seams of its 64 x 7 tiles"""
    _fused_and_standalone_steps(ocn, arch, size, substep_rides=True)


def test_flux_condition_lands_after_forcing(ocn, arch):
    """G = (G_rest + F) + flux (compute_flux_bc_tendencies! after the forcing): one forward-Euler AB2 step from a state moves T by
    Δt * G, with G formed here from the unforced tendency, F and the library's Flux-condition kernel in that order, bitwise"""
    from oldoceananigans_jl_amd import forcings as F
    size = (8, 8, 8)
    kw = dict(size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(0.37))}
    forcing = {"T": _sponge(ocn, "z", -0.1, 0.3)}
    plain, forced = _pair(ocn, arch, kw, forcing, timestepper="QuasiAdamsBashforth2", boundary_conditions=bcs)
    T0 = forced.tracers.T.interior()
    G = ocn.CenterField(forced.grid)
    G.set(plain.tendency("T").interior() + F.evaluate(forced._forcing_terms["T"], forced.grid, forced.tracers.T.loc, T0))
    ocn.compute_flux_bcs(G, bcs["T"])
    dt = 0.01
    ocn.time_step(forced, dt)
    assert np.array_equal(forced.tracers.T.interior(), T0 + dt * (1.0 * G.interior()))


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_relaxation_known_answer(ocn, arch, timestepper):
    """T ≡ 1 at rest, Relaxation(rate = 1/τ): G = -T/τ, so n RK3 steps multiply T by (1 + z + z²/2 + z³/6)^n, z = -Δt/τ; AB2 (χ = 0.1) is
    the two-step recurrence after a forward-Euler first step"""
    tau, dt, n = 3.0, 0.25, 6
    grid = ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1))
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), timestepper=timestepper, forcing={"T": ocn.Relaxation(rate=1 / tau)})
    ocn.set_model(m, T=1.0)
    for _ in range(n):
        ocn.time_step(m, dt)
    z = -dt / tau
    if timestepper == "RungeKutta3":
        want = (1 + z + z * z / 2 + z ** 3 / 6) ** n
    else:
        chi, T, Gm = 0.1, 1.0, None
        for step in range(n):
            G = -T / tau
            T = T + dt * G if step == 0 else T + dt * ((1.5 + chi) * G - (0.5 + chi) * Gm)
            Gm = G
        want = T
    T = m.tracers.T.interior()
    assert np.abs(T - want).max() <= 1e-14 * abs(want), (T.min(), T.max(), want)
    assert np.all(m.velocities.u.interior() == 0)


@pytest.mark.parametrize("mask", ["GaussianMask", "PiecewiseLinearMask"])
def test_relaxed_time_stepping(ocn, arch, mask):
    """relaxed_time_stepping (test_forcings.jl:143-157) on the smallest grid the library accepts, plus the tendency identity"""
    M = getattr(ocn, mask)
    forcing = {"u": ocn.Relaxation(rate=1 / 60, mask=M("x", center=0.5, width=0.1), target=ocn.LinearTarget("x", intercept=np.pi, gradient=np.e)),
               "v": ocn.Relaxation(rate=1 / 60, mask=M("y", center=0.5, width=0.1), target=ocn.LinearTarget("y", intercept=np.pi, gradient=np.e)),
               "w": ocn.Relaxation(rate=1 / 60, mask=M("z", center=0.5, width=0.1), target=np.pi)}
    plain, forced = _pair(ocn, arch, dict(size=(2, 2, 2), extent=(1, 1, 1)), forcing)
    _check_identity(ocn, plain, forced)
    ocn.time_step(forced, 1.0)
    assert all(np.all(np.isfinite(f.parent())) for f in forced.fields().values())


@pytest.mark.parametrize("terms", [2, 7])
def test_two_and_seven_forcings(ocn, arch, terms):
    """two_forcings / seven_forcings (test_forcings.jl:198-238): u = tuple, v = MultipleForcings(F...), w = MultipleForcings((F...)) are
    the same forcing; seven terms take the `total += Fₙ` sum"""
    size = (4, 5, 6)
    rng = np.random.default_rng(7)
    if terms == 2:
        Ft = (ocn.Relaxation(rate=1), ocn.Relaxation(rate=2))
    else:
        Ft = (ocn.Relaxation(rate=1), ocn.Forcing(rng.standard_normal(size)), _sponge(ocn, "x", 0.3, 0.2), ocn.Relaxation(rate=0.5, target=3),
              ocn.Forcing(rng.standard_normal(size)), _sponge(ocn, "y", 0.6, 0.3), _sponge(ocn, "z", -0.4, 0.2))
    forcing = {"u": Ft, "v": ocn.MultipleForcings(*Ft), "w": ocn.MultipleForcings(Ft)}
    plain, forced = _pair(ocn, arch, dict(size=size, extent=(1, 1, 1)), forcing)
    _check_identity(ocn, plain, forced)
    ocn.time_step(forced, 0.01)
    assert all(np.all(np.isfinite(f.parent())) for f in forced.fields().values())


def test_borrowed_field_forcing(ocn, arch):
    """forcing = (T = field,): the library reads the Field's memory whenever the tendency is evaluated"""
    size = (8, 8, 8)
    grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
    Fld = ocn.CenterField(grid)
    rng = np.random.default_rng(2)
    Fld.set(rng.standard_normal(size))
    plain, forced = _pair(ocn, arch, dict(size=size, extent=(1, 1, 1)), {"T": Fld})
    _check_identity(ocn, plain, forced)
    new = rng.standard_normal(size)
    Fld.set(new)
    for m in (plain, forced):
        ocn.update_state(m)
    assert np.array_equal(forced.tendency("T").interior(), plain.tendency("T").interior() + new)
    # ... and a time step uses it: with zero state and zero velocity the new forcing is the only T tendency
    ocn.set_model(forced, u=0.0, v=0.0, w=0.0, T=0.0, S=0.0)
    ocn.time_step(forced, 0.1)
    assert np.allclose(forced.tracers.T.interior(), 0.1 * new, rtol=1e-14, atol=0)


def _dist_forcing(ocn, arr):
    return {"u": _sponge(ocn, "x", 1.2, 0.3), "w": ocn.Relaxation(rate=0.8, mask=ocn.GaussianMask("z", center=-0.3, width=0.2)),
            "T": (_sponge(ocn, "z", -0.6, 0.2), _sponge(ocn, "x", 0.4, 0.5, target=1.0)), "S": arr}


@pytest.mark.parametrize("R,partition", [(2, None), (4, None), (4, (2, 2))])
def test_partitioned_matches_single_gpu(ocn, arch, R, partition):
    """x-slabs (and one 2 x 2 pencil partition) over the loopback transport: every rank forces its own interior and strips with
    rank-local tables and arrays, through the standalone pass"""
    from oldoceananigans_jl_amd import _lib, distributed as dist
    from loopback import PointerLoopbackWorld
    _lib.check(_lib.lib().ocn_own_stream())
    size, nsteps = (32, 16, 8), 3
    arr = np.random.default_rng(9).standard_normal(size)
    kw = dict(size=size, x=(0.0, 2.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    grid = ocn.RectilinearGrid(arch, **kw)
    ref = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), forcing=_dist_forcing(ocn, arr))
    vals = _state(ocn, grid, ref)
    ocn.set_model(ref, **vals)
    dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6
    for _ in range(nsteps):
        ocn.time_step(ref, dt)
    want = {n: f.parent() for n, f in ref.fields().items()}
    world = PointerLoopbackWorld(R, _lib.lib())
    results, errors = [None] * R, []
    Rx, Ry = partition or (R, 1)
    nxl, nyl = size[0] // Rx, size[1] // Ry

    def worker(rank):
        try:
            ctx = dist.Distributed.transport(arch, world.collectives(rank), R, rank)
            g = dist.DistributedRectilinearGrid(ctx, partition=partition, **kw)
            ix, iy = rank // Ry, rank % Ry
            sl = (slice(ix * nxl, (ix + 1) * nxl), slice(iy * nyl, (iy + 1) * nyl))
            m = dist.LibraryDistributedModel(grid=g, tracers=("T", "S"), forcing=_dist_forcing(ocn, arr[sl]))
            assert m.get_option("forcing_path") == 3
            ocn.set_model(m, **{n: v[sl] for n, v in vals.items()})
            for _ in range(nsteps):
                ocn.time_step(m, dt)
            results[rank] = {n: f.parent() for n, f in m.fields().items()}
            m.close()
            ctx.close()
        except BaseException as e:          # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))
            world.barrier_obj.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r, out in enumerate(results):
        ix, iy = r // Ry, r % Ry
        for n, a in out.items():
            w = want[n][3 + ix * nxl:3 + (ix + 1) * nxl, 3 + iy * nyl:3 + (iy + 1) * nyl, 3:3 + a.shape[2] - 6]
            err = np.abs(a[3:-3, 3:-3, 3:-3] - w).max() / np.abs(want[n]).max()
            assert err <= 1e-12, (r, n, err)
    ref.close()


def _oracle_forced_run(ocn, O, go, gpu_grid, terms, vals, dt, nsteps, scheme):
    """the reference's RK3 / AB2 time-step composed from the oracle's own kernels (runge_kutta_3.jl:93-170, quasi_adams_bashforth_2.jl:
    74-123, pressure_correction.jl) with the forcing term added in numpy after every tendency evaluation (G = G_rest + F)"""
    import ctypes as C
    from oldoceananigans_jl_amd import forcings as F
    from oracle.oracle import PoissonSolver
    L = O.lib()
    L.oro_ab2_step_field.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_double, C.c_double,
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]
    mo = O.Model(go, 2)
    gnames = ["u", "v", "w", "T", "S"]
    cn = ["u", "v", "w", "c0", "c1"]
    mo.set(**{c: vals[g] for c, g in zip(cn, gnames)})
    regular = not isinstance(go.dc[2], np.ndarray) or np.all(go.dc[2] == go.dc[2][0])
    kind = 0 if regular else 1
    solver = PoissonSolver(go, kind)
    U = [mo.field(c) for c in cn]
    locs = [mo.loc(c) for c in cn]
    Gn = [mo.field("G" + c) for c in cn]
    Gm = [mo.field("M" + c) for c in cn]
    gpu_locs = [tuple(ocn.Face if c else ocn.Center for c in l) for l in locs]
    p = mo.field("p")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def update_state():
        mo.update_state(True)
        for q, g in enumerate(gnames):
            if g not in terms:
                continue
            loc = gpu_locs[q]
            Gi, Ui = go.interior(Gn[q], locs[q]), go.interior(U[q], locs[q])
            r = tuple(slice(1 if (q < 3 and locs[q][d] == 1 and go.topo[d] == 1) else 0, go.N[d]) for d in range(3))
            Fq = F.evaluate(terms[g], gpu_grid, loc, Ui.copy())
            Gi[r] = Gi[r] + Fq[r]

    def pressure():
        for q in range(3):
            go.fill_halo_regions(U[q], locs[q], True)
        solver.rhs[...] = go.source_term(U[0], U[1], U[2], weight_by_dz=kind == 1)
        solver.solve(p)
        go.fill_halo_regions(p, (0, 0, 0), True)
        go.pressure_correct(U[0], U[1], U[2], p)

    def cache():
        for q in range(5):
            Gm[q][...] = Gn[q]

    update_state()
    g1, g2, g3 = 8 / 15, 5 / 12, 3 / 4
    z2, z3 = -17 / 60, -5 / 12
    for step in range(nsteps):
        if scheme == "RungeKutta3":
            for gam, zet in ((g1, None), (g2, z2), (g3, z3)):
                for q in range(5):
                    go.rk3_substep(U[q], locs[q], dt, gam, zet, Gn[q], Gm[q])
                pressure()
                if zet != z3:
                    cache()
                update_state()
        else:
            chi = -0.5 if step == 0 else 0.1
            for q in range(5):
                L.oro_ab2_step_field(go.handle, dp(U[q]), (C.c_int * 3)(*locs[q]), dt, chi, dp(Gn[q]), dp(Gm[q]))
            pressure()
            cache()
            update_state()
    return {g: go.interior(U[q], locs[q]).copy() for q, g in enumerate(gnames)}



@pytest.mark.parametrize("scheme", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("topology", ["PPP", "PPB"])
def test_time_steps_match_the_oracle_with_numpy_forcing(ocn, oracle, arch, scheme, topology):
    """5 RK3 / AB2 steps of a model with a sponge on u, v, w, T and an array forcing on S against the oracle's kernels composed with the
    same forcing in numpy, 1e-12 relative: forced velocities through the projection, forcing that varies in space across stages, AB2's
    cached forced tendency"""
    from helpers import ORACLE_TOPO, rel_err
    size = (16, 16, 16) if topology == "PPP" else (16, 16, 12)
    names = ("Periodic", "Periodic", "Periodic" if topology == "PPP" else "Bounded")
    z = (0.0, 1.0) if topology == "PPP" else tanh_faces(size[2])
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=tuple(getattr(ocn, t) for t in names))
    go = oracle.Grid(size, topology=tuple(ORACLE_TOPO[t] for t in names), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    arr = 0.1 * np.random.default_rng(4).standard_normal(size)
    forcing = {"u": _sponge(ocn, "x", 0.5, 0.2, rate=2.0), "v": _sponge(ocn, "y", 0.3, 0.2, rate=2.0, target=0.1),
               "w": ocn.Relaxation(rate=3.0, mask=ocn.GaussianMask("z", center=0.6 if topology == "PPP" else -0.4, width=0.2)),
               "T": _sponge(ocn, "z", 0.5 if topology == "PPP" else -0.5, 0.3), "S": arr}
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), timestepper=scheme, forcing=forcing)
    vals = _state(ocn, grid, m)
    ocn.set_model(m, **vals)
    dt, nsteps = 0.1 * grid.Δxᶜᵃᵃ / 0.6, 5
    for _ in range(nsteps):
        ocn.time_step(m, dt)
    want = _oracle_forced_run(ocn, oracle, go, grid, m._forcing_terms, vals, dt, nsteps, scheme)
    for n, f in m.fields().items():
        e = rel_err(f.interior(), want[n])
        assert e < 1e-12, (n, e)
