"""Relaxation with function masks and targets, and the raw evaluation of a forcing program, on the device (-m gpu;
ocn_forcing_function.h): the raw evaluation against the numpy restatement (tests/forcing_function_reference.py) with and without the
hoisted tables, the tendency identity G_forced == G_plain + F on every configuration the standalone pass serves, the function form of a
table sponge against the table form, the stage times, the captured step, the accounting, replacement and the refusals."""
import ctypes as C

import numpy as np
import pytest

import forcing_function_reference as R
from helpers import smooth_state, tanh_faces

pytestmark = pytest.mark.gpu

FIELDS = ("u", "v", "w", "T")


def _grid(ocn, arch, which):
    B, P, F = ocn.Bounded, ocn.Periodic, ocn.Flat
    if which == "A":        # more than one 64-lane tile in x with a ragged tail, an odd row count; stretched z
        return ocn.RectilinearGrid(arch, size=(70, 9, 6), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(6), topology=(B, P, B))
    if which == "B":        # Face ranges in all three directions
        return ocn.RectilinearGrid(arch, size=(12, 10, 8), x=(0.0, 1.0), y=(-0.5, 0.5), z=(-1.0, 0.0), topology=(B, B, B))
    return ocn.RectilinearGrid(arch, size=(16, 8), x=(0.0, 2.0), z=(-1.0, 0.0), topology=(P, F, B))


def _random_fields(ocn, grid, rng, low=-1.0, high=1.0, names=FIELDS):
    from oldoceananigans_jl_amd.boundary_functions import assumed_field_location
    fields, parents = {}, {}
    for name in names:
        f = ocn.Field(assumed_field_location(name), grid)
        f.set_parent(rng.uniform(low, high, f.shape))
        ocn.fill_halo_regions(f)
        fields[name], parents[name] = f, f.parent()
    return fields, parents


def _ncoords(ocn, grid):
    return sum(t is not ocn.Flat for t in grid.topology)


def _with_coordinates(f, n):
    """f(X, t, deps...) as a function of the reference's signature for a grid with n coordinates"""
    return lambda *a: f(a[:n], a[n], *a[n + 1:])


def _raw(ocn, grid, func, loc, deps, t):
    """(device with tables, device without, restatement) of func at loc; deps: (Field, host parent) pairs"""
    from oldoceananigans_jl_amd import boundary_functions as BF
    coords = [d for d in range(3) if grid.topology[d] is not ocn.Flat]
    program = BF.trace(func, coords, len(deps))
    hoisted = ocn.kernels.evaluate_forcing_function(grid, program, loc, [f for f, _ in deps], t, hoist=True)
    whole = ocn.kernels.evaluate_forcing_function(grid, program, loc, [f for f, _ in deps], t, hoist=False)
    ref = R.evaluate(func, grid, loc, [(p, f.loc) for f, p in deps], t)
    return hoisted, whole, ref


# ---------------------------------------------------------------------------------------------------------------------
# 1. raw evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_exact_programs_equal_the_restatement(ocn, arch, which):
    """coordinates, t, ifelse / min / max and dependencies interpolated in one and in two directions, at the locations of u, v, w, T: the
    whole interior ==, with the tables == without them"""
    from oldoceananigans_jl_amd.boundary_functions import assumed_field_location
    grid = _grid(ocn, arch, which)
    rng = np.random.default_rng(11)
    fields, parents = _random_fields(ocn, grid, rng)
    first = lambda X: X[0]                                                                               # noqa: E731
    last = lambda X: X[-1]                                                                               # noqa: E731
    functions = [lambda X, t, u, v, w, T: first(X) * last(X) + t * u - v / (1.5 + w * T),
                 lambda X, t, u, v, w, T: ocn.ifelse(w > u, ocn.min_(u, first(X)), ocn.max_(v, T)) + abs(w) * (T >= 0.25) - last(X) / 3.0,
                 lambda X, t, u, v, w, T: (1.0 + first(X) * first(X)) * (last(X) - t) * T,              # f(x) g(z) φ: two line roots
                 lambda X, t, u, v, w, T: last(X) * 2.0 + t]                                             # the result is a line value
    n = _ncoords(ocn, grid)
    deps = [(fields[d], parents[d]) for d in FIELDS]
    for name in FIELDS:
        for q, f in enumerate(functions):
            hoisted, whole, ref = _raw(ocn, grid, _with_coordinates(f, n), assumed_field_location(name), deps, 1.75)
            assert hoisted.shape == ref.shape == tuple(grid.interior_size(assumed_field_location(name)))
            assert np.array_equal(hoisted, ref), (which, name, q, np.abs(hoisted - ref).max())
            assert np.array_equal(whole, hoisted), (which, name, q)
            assert np.unique(ref).size > 1


def test_dependency_interpolated_in_three_directions(ocn, arch):
    grid = _grid(ocn, arch, "B")
    rng = np.random.default_rng(5)
    corner = ocn.Field((ocn.Face, ocn.Face, ocn.Face), grid)
    corner.set_parent(rng.uniform(-1.0, 1.0, corner.shape))
    centre = ocn.CenterField(grid)
    centre.set_parent(rng.uniform(-1.0, 1.0, centre.shape))
    for dep, loc in ((corner, centre.loc), (centre, corner.loc)):
        hoisted, whole, ref = _raw(ocn, grid, lambda x, y, z, t, a: a * (x + y) - z, loc, [(dep, dep.parent())], 0.0)
        assert np.array_equal(hoisted, ref) and np.array_equal(whole, ref)


# units in the last place: OpenCL's double-precision bounds for exp, log, sin, cos, tanh, pow (the ROCm installation carries no accuracy
# table of its device math library) plus 1 ulp for numpy's own error
ULP_BOUNDS = {"exp": 3 + 1, "log": 3 + 1, "sin": 4 + 1, "cos": 4 + 1, "tanh": 5 + 1, "pow": 16 + 1}


def test_transcendental_programs_within_the_documented_ulps(ocn, arch):
    """exp, sin, cos, tanh on [-10, 10], log on [1e-3, 10], pow with base in [0.1, 10] and exponent in [-3, 3] on grid A, at T's location
    (identity) and at u's (interpolated arguments): |device - numpy| in ulps of the numpy value; the tables change nothing"""
    from oldoceananigans_jl_amd.boundary_functions import assumed_field_location
    grid = _grid(ocn, arch, "A")
    rng = np.random.default_rng(13)
    wide = _random_fields(ocn, grid, rng, -10.0, 10.0, ("T",))
    positive = _random_fields(ocn, grid, rng, 1e-3, 10.0, ("T",))
    base = _random_fields(ocn, grid, rng, 0.1, 10.0, ("T",))
    expo = _random_fields(ocn, grid, rng, -3.0, 3.0, ("T",))
    pair = lambda s: [(s[0]["T"], s[1]["T"])]                                                            # noqa: E731
    cases = {"exp": (lambda x, y, z, t, T: ocn.exp(T), pair(wide)), "sin": (lambda x, y, z, t, T: ocn.sin(T), pair(wide)),
             "cos": (lambda x, y, z, t, T: ocn.cos(T), pair(wide)), "tanh": (lambda x, y, z, t, T: ocn.tanh(T), pair(wide)),
             "log": (lambda x, y, z, t, T: ocn.log(T), pair(positive)), "pow": (lambda x, y, z, t, b, e: b ** e, pair(base) + pair(expo))}
    worst = {}
    for name in ("T", "u"):
        for op, (f, deps) in cases.items():
            hoisted, whole, ref = _raw(ocn, grid, f, assumed_field_location(name), deps, 0.0)
            assert np.array_equal(hoisted, whole), op
            worst[op] = max(worst.get(op, 0.0), float(np.max(np.abs(hoisted - ref) / np.spacing(np.abs(ref)))))
    print("largest difference in ulps:", {k: round(v, 3) for k, v in worst.items()})
    for op, bound in ULP_BOUNDS.items():
        assert worst[op] <= bound, (op, worst[op], bound)


def test_raw_entry_point_refuses_before_any_launch(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import boundary_functions as BF
    OP = BF.OPS
    grid, flat = _grid(ocn, arch, "A"), _grid(ocn, arch, "C")
    T, out = ocn.CenterField(grid), ocn.CenterField(grid)
    Tf, outf = ocn.CenterField(flat), ocn.CenterField(flat)
    good = [(OP["field"], 0, 0, 0, 0.0), (OP["coord"], 2, 0, 0, 0.0), (OP["*"], 0, 1, 0, 0.0)]

    def status(program, g=grid, dep=T, o=out, ndeps=1, n=None):
        arr, m = BF.program_array(program)
        ptrs = (C.c_void_p * 1)(dep.data)
        locs = ((C.c_int * 3) * 1)()
        return _lib.lib().ocn_evaluate_forcing_function(g.handle, arr, m if n is None else n, _lib.i3((0, 0, 0)), ptrs, locs, ndeps, 0.0, 1, o.data)
    assert status(good) == 0
    assert status(good, n=0) == -1 and status(good + [(OP["const"], 0, 0, 0, 0.0)] * 62, n=65) == -1
    assert status([(OP["field"], 0, 0, 0, 0.0), (OP["*"], 0, 1, 0, 0.0)]) == -1
    assert status([(99, 0, 0, 0, 0.0)]) == -1 and status([(24, 0, 0, 0, 0.0)]) == -1                 # the table load is not a public op
    assert status([(OP["field"], 1, 0, 0, 0.0)]) == -1 and status(good, ndeps=0) == -1
    assert status([(OP["coord"], 3, 0, 0, 0.0)]) == -1
    assert status(good, g=flat, dep=Tf, o=outf) == 0
    assert status([(OP["coord"], 1, 0, 0, 0.0)], g=flat, dep=Tf, o=outf) == -1 and b"Flat" in _lib.lib().ocn_last_error()
    # eight dependencies at the most
    ptrs, locs = (C.c_void_p * 9)(*[T.data] * 9), ((C.c_int * 3) * 9)()
    arr, m = BF.program_array(good)
    assert _lib.lib().ocn_evaluate_forcing_function(grid.handle, arr, m, _lib.i3((0, 0, 0)), ptrs, locs, 8, 0.0, 1, out.data) == 0
    assert _lib.lib().ocn_evaluate_forcing_function(grid.handle, arr, m, _lib.i3((0, 0, 0)), ptrs, locs, 9, 0.0, 1, out.data) == -1
    assert b"dependencies" in _lib.lib().ocn_last_error()
    # a grid without node tables: OCN_ESTATE (the host mirror always hands them over, so the handle is made here)
    bare = C.c_void_p()
    _lib.check(_lib.lib().ocn_grid_create(C.byref(bare), _lib.i3((8, 8, 8)), _lib.i3((3, 3, 3)), _lib.i3((0, 0, 0)), (C.c_double * 3)(1.0, 1.0, 1.0),
                                          0.125, 0.125, 0.125, None, None))
    small = ocn.CenterField(ocn.RectilinearGrid(arch, size=(8, 8, 8), extent=(1, 1, 1)))
    arr, m = BF.program_array([(OP["const"], 0, 0, 0, 1.0)])
    assert _lib.lib().ocn_evaluate_forcing_function(bare, arr, m, _lib.i3((0, 0, 0)), None, None, 0, 0.0, 1, small.data) == -3
    assert b"ocn_grid_set_node_tables" in _lib.lib().ocn_last_error()
    _lib.check(_lib.lib().ocn_grid_destroy(bare))
    from oldoceananigans_jl_amd import distributed as dist
    uid = C.create_string_buffer(128)
    _lib.check(_lib.lib().ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    pgrid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    arr, m = BF.program_array([(OP["const"], 0, 0, 0, 1.0)])
    assert _lib.lib().ocn_evaluate_forcing_function(pgrid.local.handle, arr, m, _lib.i3((0, 0, 0)), None, None, 0, 0.0, 1, out.data) == -2
    assert b"partitioned" in _lib.lib().ocn_last_error()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the tendency identity
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_range(grid, loc, ocn, velocity):
    """the interior range the tendency launch covers: the first Face index of a Bounded direction is excluded for velocities"""
    return tuple(slice(1 if (velocity and l is ocn.Face and t is ocn.Bounded and grid.size[d] > 1) else 0, grid.size[d])
                 for d, (l, t) in enumerate(zip(loc, grid.topology)))


def _state(grid, model, seed=3):
    return smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed)


def _pair(ocn, arch, make_grid, forcing, t0=0.0, **model_kw):
    from oldoceananigans_jl_amd import _lib
    models = []
    for frc in (None, forcing):
        m = ocn.NonhydrostaticModel(grid=make_grid(), tracers=("T", "S"), forcing=frc, **model_kw)
        models.append(m)
    vals = _state(models[0].grid, models[0])
    for m in models:
        ocn.set_model(m, **vals)
        _lib.check(_lib.lib().ocn_model_set_clock(m.handle, t0, 0, 1, float("inf"), float("inf")))
        ocn.update_state(m)
    return models


def _check_identity(ocn, plain, forced, t):
    from oldoceananigans_jl_amd import forcings as F
    grid = forced.grid
    for name, fld in forced.fields().items():
        G0, G1 = plain.tendency(name).interior(), forced.tendency(name).interior()
        terms = forced._forcing_terms.get(name)
        if not terms:
            assert np.array_equal(G0, G1), name
            continue
        want = G0.copy()
        r = _kernel_range(grid, fld.loc, ocn, name in ("u", "v", "w"))
        want[r] = G0[r] + F.evaluate(terms, grid, fld.loc, fld.interior(), t=t)[r]
        assert np.array_equal(G1, want), (name, np.abs(G1 - want).max())
        assert np.abs(want - G0).max() > 0, name


def _exact_forcings(ocn, grid, rng, flat):
    """exact-operation masks and targets (numpy's exp and the device's differ in the last place): two walls at once, a lateral sponge that
    fades with depth, a target that moves in time; a 3-term and a 5-term sum with a function, an array and a built-in relaxation"""
    arr = rng.standard_normal(grid.size)
    west = lambda x: ocn.max_(0.0, 1.0 - abs(x - 0.1) / 0.4)                                            # noqa: E731
    deep = lambda z: ocn.max_(0.0, 1.0 - abs(z + 0.9) / 0.5)                                            # noqa: E731
    if flat:
        two_walls = ocn.Relaxation(rate=0.7, mask=lambda x, z: ocn.max_(west(x), deep(z)), target=lambda x, z, t: 0.3 + 0.2 * z * t)
        fading = ocn.Relaxation(rate=0.4, mask=lambda x, z: west(x) * (1.0 + z) * (1.0 + z))
        moving = ocn.Relaxation(rate=0.9, target=lambda x, z, t: ocn.ifelse(x > 0.5, t, -t) / (2.0 + z))
    else:
        two_walls = ocn.Relaxation(rate=0.7, mask=lambda x, y, z: ocn.max_(west(x), deep(z)), target=lambda x, y, z, t: 0.3 + 0.2 * z * t)
        fading = ocn.Relaxation(rate=0.4, mask=lambda x, y, z: west(x) * (1.0 + z) * (1.0 + z) + 0.1 * y)
        moving = ocn.Relaxation(rate=0.9, target=lambda x, y, z, t: ocn.ifelse(x > 0.5, t, -t) / (2.0 + z * y))
    table = ocn.Relaxation(rate=0.2, mask=ocn.PiecewiseLinearMask("x", center=0.7, width=0.5), target=ocn.LinearTarget("z", intercept=0.3, gradient=0.2))
    return {"u": two_walls, "v": (fading, ocn.Forcing(arr), table), "w": moving,
            "T": ocn.MultipleForcings(table, two_walls, ocn.Forcing(arr), ocn.Relaxation(rate=0.05, target=2.0), moving),
            "S": table}                                                              # (no function term: stays with the standalone table pass)


CASES = [("triply periodic", "PPP", {}), ("marching epilogue", "PPB", {"closure": True}), ("per-value epilogue", "PPB", {"coriolis": True}),
         ("per-field kernels", "BPB", {}), ("Flat y", "PFB", {})]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tendency_identity_bitwise(ocn, arch, case):
    _, topology, physics = case
    names = {"P": ocn.Periodic, "B": ocn.Bounded, "F": ocn.Flat}
    topo = tuple(names[t] for t in topology)
    flat = topology[1] == "F"
    size = (70, 6) if flat else (70, 9, 6)
    kw = dict(size=size, x=(0.0, 1.0), z=tanh_faces(6) if topology[2] == "B" else (-1.0, 0.0), topology=topo)
    if not flat:
        kw["y"] = (0.0, 1.0)
    model_kw = {}
    if physics.get("coriolis"):
        model_kw["coriolis"] = ocn.FPlane(f=0.7)
    if physics.get("closure"):
        model_kw["closure"] = ocn.ScalarDiffusivity(ν=1e-3, κ=2e-3)
    make = lambda: ocn.RectilinearGrid(arch, **kw)                                                       # noqa: E731
    forcing = _exact_forcings(ocn, make(), np.random.default_rng(11), flat)
    plain, forced = _pair(ocn, arch, make, forcing, t0=1.75, **model_kw)
    assert plain.get_option("forcing_path") == 0 and forced.get_option("forcing_path") == 3
    assert forced.get_option("forcing_functions") == 5 and forced.get_option("forcing_functions_read_time") == 1
    assert forced.get_option("fuse_substep_active") == 0
    _check_identity(ocn, plain, forced, 1.75)
    forced.set_option("forcing_function_hoist", 0)
    ocn.update_state(forced)
    _check_identity(ocn, plain, forced, 1.75)
    plain.close()
    forced.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the function form of a table sponge
# ---------------------------------------------------------------------------------------------------------------------
def _run(ocn, model, steps, dt):
    for _ in range(steps):
        ocn.time_step(model, dt)
    return {n: f.parent() for n, f in model.fields().items()} | {"p": model.pressures.pNHS.parent()}


@pytest.mark.parametrize("stepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_function_form_equals_table_form(ocn, arch, stepper):
    """a PiecewiseLinearMask + LinearTarget sponge on all five fields written as functions == the built-in model on its standalone pass,
    every field after 3 steps: the same operations per node and per cell"""
    c, w, a, b, rate = -0.8, 0.4, 0.3, 0.2, 1.5
    table = ocn.Relaxation(rate=rate, mask=ocn.PiecewiseLinearMask("z", center=c, width=w), target=ocn.LinearTarget("z", intercept=a, gradient=b))
    function = ocn.Relaxation(rate=rate, mask=lambda x, y, z: ocn.max_(0.0, 1.0 - abs(z - c) / w), target=lambda x, y, z, t: a + b * z)
    out = []
    for sponge in (table, function):
        grid = _grid(ocn, arch, "A")
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), timestepper=stepper, forcing={n: sponge for n in ("u", "v", "w", "T", "S")})
        model.set_option("fused_forcing", 0)
        assert model.get_option("forcing_path") == 3 and model.get_option("forcing_functions") == (5 if sponge is function else 0)
        if sponge is function:              # two table loads, the field, a subtraction and a multiplication
            assert model.get_option("forcing_function_cell_instructions") == 5
        ocn.set_model(model, **_state(grid, model, seed=5))
        out.append(_run(ocn, model, 3, 0.05 * grid.Δxᶜᵃᵃ))
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n
    assert np.isfinite(out[0]["T"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. stage times
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_time_dependent_target_sees_the_stage_times(ocn, arch, stepper):
    """target(x, y, z, t) = t on a uniform tracer at rest: G = rate (t - T) with t the clock of each tendency evaluation -- tⁿ, tⁿ + γ¹Δt,
    tⁿ + (γ¹ + γ² + ζ²)Δt in RK3 (runge_kutta_3.jl:93-170), tⁿ in AB2 -- replayed on the host. A wrong stage time shows at O(Δt²) = 1e-2;
    the round-off of the handful of O(1) operations is below 1e-15. The step is never replayed from a graph."""
    from oldoceananigans_jl_amd import _lib
    grid = _grid(ocn, arch, "B")
    rate, t0, T0, dt, steps = 0.8, 2.5, 1.0, 0.1, 2
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), timestepper=stepper, forcing={"T": ocn.Relaxation(rate=rate, target=lambda x, y, z, t: t)})
    model.set_option("use_graph", 1)
    assert model.get_option("forcing_functions_read_time") == 1
    ocn.set_model(model, T=T0)
    _lib.check(_lib.lib().ocn_model_set_clock(model.handle, t0, 0, 1, float("inf"), float("inf")))
    for _ in range(steps):
        ocn.time_step(model, dt)
    G = lambda t, T: rate * (t - T)                                                                      # noqa: E731
    t, T, Gm = t0, T0, None
    for step in range(steps):
        if stepper == "RungeKutta3":
            g1, g2, g3, z2, z3 = 8 / 15, 5 / 12, 3 / 4, -17 / 60, -5 / 12
            G0 = G(t, T)
            T = T + dt * g1 * G0
            t1 = t + dt * g1
            G1 = G(t1, T)
            T = T + dt * (g2 * G1 + z2 * G0)
            t2 = t1 + dt * (g2 + z2)
            T = T + dt * (g3 * G(t2, T) + z3 * G1)
            t = t + dt
        else:
            chi = -0.5 if step == 0 else 0.1
            Gn = G(t, T)
            T = T + dt * ((1.5 + chi) * Gn - (0.5 + chi) * (Gm if Gm is not None else 0.0))
            Gm, t = Gn, t + dt
    got = model.tracers.T.interior()
    print("T:", got[0, 0, 0], "expected", T, "difference", abs(got[0, 0, 0] - T))
    assert np.all(np.abs(got - T) <= 1e-13)
    assert abs(T - T0) > 0.1 and abs(model.clock.time - (t0 + steps * dt)) < 1e-12
    for _ in range(4):
        ocn.time_step(model, dt)
    assert model.get_option("graph_replays") == 0 and model.get_option("graph_captures") == 0
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. graph, accounting, replacement
# ---------------------------------------------------------------------------------------------------------------------
def _sponge_model(ocn, grid, **kw):
    sponge = ocn.Relaxation(rate=1.5, mask=lambda x, y, z: ocn.max_(ocn.exp(-(x - 0.5) ** 2 / 0.02), ocn.exp(-(z + 0.9) ** 2 / 0.02)),
                            target=lambda x, y, z, t: ocn.tanh(z / 0.3))
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), forcing={"u": sponge, "T": sponge}, **kw)
    ocn.set_model(model, **_state(grid, model, seed=9))
    return model


def test_time_free_functions_keep_the_captured_step(ocn, arch):
    out = []
    for use_graph in (1, 0):
        grid = _grid(ocn, arch, "B")
        model = _sponge_model(ocn, grid)
        model.set_option("use_graph", use_graph)
        assert model.get_option("forcing_functions_read_time") == 0
        out.append(_run(ocn, model, 6, 0.02 * grid.Δxᶜᵃᵃ))
        assert (model.get_option("graph_replays") > 0) == bool(use_graph)
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


def test_hoisting_changes_no_bit_over_time_steps(ocn, arch):
    out = []
    for hoist in (1, 0):
        grid = _grid(ocn, arch, "A")
        model = _sponge_model(ocn, grid)
        assert model.get_option("forcing_function_hoist") == 1
        model.set_option("forcing_function_hoist", hoist)
        n = model.get_option("forcing_function_cell_instructions")
        assert (n < 12) if hoist else (n > 20), n            # the mixed max(exp, exp) mask: two loads and a max instead of both Gaussians
        # ... so no transcendental is left per cell and the arithmetic-only instantiation of the kernel runs; the recorded program needs the full one
        assert model.get_option("forcing_function_arithmetic_only") == hoist
        out.append(_run(ocn, model, 3, 0.02 * grid.Δxᶜᵃᵃ))
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


def test_node_tables_are_rewritten_in_place(ocn, arch):
    """the programs of a model hold addresses inside the grid's node tables: a later ocn_grid_set_node_tables writes the same block, so
    the recorded program at every cell (hoist 0) keeps reading valid coordinates"""
    from oldoceananigans_jl_amd import _lib
    out = []
    for again in (False, True):
        grid = _grid(ocn, arch, "B")
        model = _sponge_model(ocn, grid)
        model.set_option("forcing_function_hoist", 0)
        ocn.time_step(model, 0.02 * grid.Δxᶜᵃᵃ)
        if again:
            dp = C.POINTER(C.c_double)
            tables = [(dp * 3)(*[a.ctypes.data_as(dp) for a in t]) for t in grid._node_tables]
            _lib.check(_lib.lib().ocn_grid_set_node_tables(grid.handle, tables[0], tables[1]))
        out.append(_run(ocn, model, 2, 0.02 * grid.Δxᶜᵃᵃ))
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


def test_replacement_and_clearing(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import forcings as F
    L = _lib.lib()
    grid, plain_grid = _grid(ocn, arch, "B"), _grid(ocn, arch, "B")
    model = _sponge_model(ocn, grid)
    plain = ocn.NonhydrostaticModel(grid=plain_grid, tracers=("T",))
    ocn.set_model(plain, **_state(plain_grid, plain, seed=9))
    count = lambda m: (m.get_option("forcing_functions"), m.get_option("forcing_path"))                # noqa: E731
    assert count(model) == (2, 3) and count(plain) == (0, 0)
    # a function replaces a function; a table relaxation replaces it and the other field keeps its own; clearing both leaves the plain model
    locs = {"u": (ocn.Face, ocn.Center, ocn.Center), "T": (ocn.Center, ocn.Center, ocn.Center)}
    keep = []
    other = F.model_forcing(grid, locs, {"T": ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x * z)})["T"]
    F.set_forcing(model.handle, 3, other, grid, keep, model._cname)
    assert count(model) == (2, 3) and model.get_option("forcing_function_cell_instructions") >= 5
    F.set_forcing(model.handle, 3, F.model_forcing(grid, locs, {"T": ocn.Relaxation(rate=1.0)})["T"], grid, keep)
    assert count(model) == (1, 3)
    # refused terms change nothing: an unknown dependency, a coordinate other than x / y / z, an operand that is no earlier value
    bad = [F.Term(3, program=other[0].program, dep_names=("q",)), F.Term(3, program=[(1, 3, 0, 0, 0.0)], dep_names=()),
           F.Term(3, program=[(6, 0, 0, 0, 0.0)], dep_names=()), F.Term(3, program=other[0].program, dep_names=("u",) * 9)]
    for term in bad:
        with pytest.raises(ocn.OcnError):
            F.set_forcing(model.handle, 0, [term], grid, keep)
    assert count(model) == (1, 3)
    # sixteen functions per model: u carries one, so 8 + 7 more fit and an eighth on w does not
    eight = other * 8
    F.set_forcing(model.handle, 1, eight, grid, keep, lambda n: "v")
    F.set_forcing(model.handle, 2, other * 7, grid, keep, lambda n: "w")
    assert count(model) == (16, 3)
    with pytest.raises(ocn.OcnError, match="16"):
        F.set_forcing(model.handle, 2, eight, grid, keep, lambda n: "w")
    assert count(model) == (16, 3)
    for f in range(4):
        _lib.check(L.ocn_model_set_forcing(model.handle, f, None, 0))
    assert count(model) == (0, 0)
    dt = 0.02 * grid.Δxᶜᵃᵃ
    a, b = _run(ocn, model, 2, dt), _run(ocn, plain, 2, dt)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    model.close()
    plain.close()


def test_partitioned_models_refuse_functions(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import distributed as dist
    from oldoceananigans_jl_amd import forcings as F
    L = _lib.lib()
    uid = C.create_string_buffer(128)
    _lib.check(L.ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    grid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    part = dist.LibraryDistributedModel(grid=grid, tracers=("T",))
    term = F.Term(3, program=[(0, 0, 0, 0, 1.0)], dep_names=())
    with pytest.raises(ocn.OcnError, match="partitioned"):
        F.set_forcing(part.handle, 3, [term], grid.local, [])
    assert part.get_option("forcing_functions") == 0 and part.get_option("forcing_path") == 0
    with pytest.raises(NotImplementedError, match="partitioned"):
        dist.LibraryDistributedModel(grid=grid, tracers=("T",), forcing={"T": ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x)})
    part.close()
    ctx.close()
