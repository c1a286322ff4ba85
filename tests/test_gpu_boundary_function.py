"""FluxBoundaryCondition(func, field_dependencies, parameters) on the device (-m gpu): the raw evaluation against the numpy restatement
(tests/boundary_function_reference.py), the linear family against the LinearFieldFlux conditions the oracle tests hold, the quadratic
bottom drag against a twin with array-valued conditions, the RK3 stage times, the captured step, replacement and accounting."""
import ctypes as C

import numpy as np
import pytest

import boundary_function_reference as R
from helpers import smooth_state, tanh_faces

pytestmark = pytest.mark.gpu

SIDES = R.SIDES
FIELDS = ("u", "v", "w", "T")


def _grid(ocn, arch, which):
    B, P, F = ocn.Bounded, ocn.Periodic, ocn.Flat
    if which == "A":        # a 70-point edge crosses a wave boundary; stretched z
        return ocn.RectilinearGrid(arch, size=(70, 9, 6), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(6), topology=(B, P, B))
    if which == "B":
        return ocn.RectilinearGrid(arch, size=(12, 10, 8), x=(0.0, 1.0), y=(-0.5, 0.5), z=(-1.0, 0.0), topology=(B, B, B))
    return ocn.RectilinearGrid(arch, size=(16, 8), x=(0.0, 2.0), z=(-1.0, 0.0), topology=(P, F, B))


def _walls(ocn, grid):
    return [s for s in range(6) if grid.topology[s // 2] is ocn.Bounded]


def _random_fields(ocn, grid, rng, low=-1.0, high=1.0):
    """u, v, w, T with random interiors and filled halos; returns the Fields and their host parents"""
    from oldoceananigans_jl_amd.boundary_functions import assumed_field_location
    fields, parents = {}, {}
    for name in FIELDS:
        f = ocn.Field(assumed_field_location(name), grid)
        f.set_parent(rng.uniform(low, high, f.shape))
        ocn.fill_halo_regions(f)
        fields[name], parents[name] = f, f.parent()
    return fields, parents


def _ncoords(ocn, grid, side):
    from oldoceananigans_jl_amd.boundary_functions import tangential_directions
    return sum(grid.topology[q] is not ocn.Flat for q in tangential_directions(side))


def _with_coordinates(f, n):
    """f(X, t, u, v, w, T) as a function of the reference's signature for a boundary with n coordinates"""
    return lambda *a: f(a[:n], a[n], *a[n + 1:])


def _raw(ocn, grid, func, name, side, fields, parents, t, parameters=None):
    """(device, restatement) of func for a condition at the location of `name` on `side`, with the dependencies u, v, w, T"""
    from oldoceananigans_jl_amd import boundary_functions as BF
    loc = BF.assumed_field_location(name)
    rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(func, parameters, FIELDS), grid, loc, side, FIELDS)
    dev = ocn.kernels.evaluate_boundary_function(grid, rbf.program, loc, side, [fields[n] for n in FIELDS], t)
    with np.errstate(all="ignore"):
        ref = R.evaluate(func, grid, loc, side, [(parents[n], BF.assumed_field_location(n)) for n in FIELDS], t, parameters)
    return dev, ref


# ---------------------------------------------------------------------------------------------------------------------
# 1. raw evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_exact_programs_equal_the_restatement(ocn, arch, which):
    """drag, a + b φ, ifelse / min / max, coordinates and t on every wall side, for conditions at the locations of u, v, w, T: ==, whole array"""
    grid = _grid(ocn, arch, which)
    rng = np.random.default_rng(11)
    fields, parents = _random_fields(ocn, grid, rng)
    cD, V = 2e-3, 0.1
    first = lambda X: X[0] if X else 1.0                                                               # noqa: E731
    last = lambda X: X[-1] if X else 0.25                                                              # noqa: E731
    functions = [lambda X, t, u, v, w, T: -cD * ocn.sqrt(u ** 2 + (v + V) ** 2) * u,
                 lambda X, t, u, v, w, T: 1e-4 + (-2.5e-3) * T,
                 lambda X, t, u, v, w, T: ocn.ifelse(w > u, ocn.min_(u, v), ocn.max_(v, T)) + t * first(X) - last(X) / 3.0 + abs(w) * (T >= 0.25),
                 lambda X, t, u, v, w, T: (first(X) - t) ** 2 / (1.5 + u * w) - ocn.ifelse(v <= T, -T, last(X) * t)]
    checked = varied = 0
    for side in _walls(ocn, grid):
        n = _ncoords(ocn, grid, side)
        for name in FIELDS:
            for q, f in enumerate(functions):
                dev, ref = _raw(ocn, grid, _with_coordinates(f, n), name, side, fields, parents, 1.75)
                assert dev.shape == ref.shape and np.array_equal(dev, ref), (which, SIDES[side], name, q)
                varied += np.unique(ref).size > 1                        # (u is 0 on its own wall: the drag there is -0 everywhere)
                checked += 1
    assert checked == {"A": 4, "B": 6, "C": 2}[which] * 4 * 4 and varied > 0.8 * checked


# units in the last place: OpenCL's double-precision bounds for exp, log, sin, cos, tanh, pow (the ROCm installation carries no accuracy
# table of its device math library) plus 1 ulp for numpy's own error
ULP_BOUNDS = {"exp": 3 + 1, "log": 3 + 1, "sin": 4 + 1, "cos": 4 + 1, "tanh": 5 + 1, "pow": 16 + 1}


def test_transcendental_programs_within_the_documented_ulps(ocn, arch):
    """exp, sin, cos, tanh on [-10, 10], log on [1e-3, 10], pow with base in [0.1, 10] and exponent in [-3, 3], on grid A's top and west sides,
    at T's location (identity) and at u's (interpolated arguments): |device - numpy| in ulps of the numpy value"""
    grid = _grid(ocn, arch, "A")
    rng = np.random.default_rng(13)
    wide, wide_p = _random_fields(ocn, grid, rng, -10.0, 10.0)
    positive, positive_p = _random_fields(ocn, grid, rng, 1e-3, 10.0)
    base, base_p = _random_fields(ocn, grid, rng, 0.1, 10.0)
    expo, expo_p = _random_fields(ocn, grid, rng, -3.0, 3.0)
    cases = {"exp": (lambda X, t, u, v, w, T: ocn.exp(T), wide, wide_p), "sin": (lambda X, t, u, v, w, T: ocn.sin(T), wide, wide_p),
             "cos": (lambda X, t, u, v, w, T: ocn.cos(T), wide, wide_p), "tanh": (lambda X, t, u, v, w, T: ocn.tanh(T), wide, wide_p),
             "log": (lambda X, t, u, v, w, T: ocn.log(T), positive, positive_p)}
    worst = {}
    for side in (5, 0):
        n = _ncoords(ocn, grid, side)
        for name in ("T", "u"):
            for op, (f, fields, parents) in cases.items():
                dev, ref = _raw(ocn, grid, _with_coordinates(f, n), name, side, fields, parents, 0.0)
                worst[op] = max(worst.get(op, 0.0), float(np.max(np.abs(dev - ref) / np.spacing(np.abs(ref)))))
            # pow: the base and the exponent are two centre fields
            from oldoceananigans_jl_amd import boundary_functions as BF
            loc, ccc = BF.assumed_field_location(name), BF.assumed_field_location("T")
            f = _with_coordinates(lambda X, t, b, e: b ** e, n)
            program = BF.trace(f, [0, 1], 2)
            dev = ocn.kernels.evaluate_boundary_function(grid, program, loc, side, [base["T"], expo["T"]], 0.0)
            ref = R.evaluate(f, grid, loc, side, [(base_p["T"], ccc), (expo_p["T"], ccc)], 0.0)
            worst["pow"] = max(worst.get("pow", 0.0), float(np.max(np.abs(dev - ref) / np.spacing(np.abs(ref)))))
    print("largest difference in ulps:", {k: round(v, 3) for k, v in worst.items()})
    for op, bound in ULP_BOUNDS.items():
        assert worst[op] <= bound, (op, worst[op], bound)


def test_raw_entry_point_refuses_before_any_launch(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import boundary_functions as BF
    OP = BF.OPS
    grid = _grid(ocn, arch, "A")
    T = ocn.CenterField(grid)
    out = ocn.CenterField(grid)                                    # (more than Na * Nb doubles)
    good = [(OP["field"], 0, 0, 0, 0.0), (OP["const"], 0, 0, 0, 2.0), (OP["*"], 0, 1, 0, 0.0)]
    loc = (ocn.Center, ocn.Center, ocn.Center)

    def status(program, side=5, ndeps=1, n=None):
        arr, m = BF.program_array(program)
        ptrs = (C.c_void_p * 1)(T.data)
        locs = ((C.c_int * 3) * 1)()
        return _lib.lib().ocn_evaluate_boundary_function(grid.handle, arr, m if n is None else n, _lib.i3((0, 0, 0)), side, ptrs, locs, ndeps, 0.0, out.data)
    assert status(good) == 0
    assert status(good, n=0) == -1 and status(good + [(OP["const"], 0, 0, 0, 0.0)] * 62, n=65) == -1                 # n outside 1..64
    assert status([(OP["field"], 0, 0, 0, 0.0), (OP["*"], 0, 1, 0, 0.0)]) == -1                                        # an operand that is not earlier
    assert status([(OP["field"], 0, 0, 0, 0.0), (OP["neg"], 1, 0, 0, 0.0)]) == -1
    assert status([(OP["field"], 0, 0, 0, 0.0), (OP["select"], 0, 0, 2, 0.0)]) == -1
    assert status([(99, 0, 0, 0, 0.0)]) == -1 and status([(-1, 0, 0, 0, 0.0)]) == -1                                 # an unknown op
    assert status([(OP["field"], 1, 0, 0, 0.0)]) == -1 and status(good, ndeps=0) == -1                               # a slot >= ndeps
    assert status([(OP["coord"], 2, 0, 0, 0.0)]) == -1
    assert status(good, side=2) == -1 and status(good, side=3) == -1 and status(good, side=6) == -1                  # y is Periodic: no wall
    assert b"wall" in _lib.lib().ocn_last_error() or b"side" in _lib.lib().ocn_last_error()
    with pytest.raises(ocn.OcnError):
        ocn.kernels.evaluate_boundary_function(grid, good, loc, "south", [T], 0.0)
    # a connected topology: OCN_ENOTSUP
    from oldoceananigans_jl_amd import distributed as dist
    uid = C.create_string_buffer(128)
    _lib.check(_lib.lib().ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    pgrid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    arr, m = BF.program_array([(OP["const"], 0, 0, 0, 1.0)])
    assert _lib.lib().ocn_evaluate_boundary_function(pgrid.local.handle, arr, m, _lib.i3((0, 0, 0)), 5, None, None, 0, 0.0, out.data) == -2
    assert b"partitioned" in _lib.lib().ocn_last_error()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the linear family, pinned through the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _run(ocn, model, steps, dt):
    for _ in range(steps):
        ocn.time_step(model, dt)
    return {n: f.parent() for n, f in model.fields().items()} | {"p": model.pressures.pNHS.parent()}


@pytest.mark.parametrize("stepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("path", [{}, {"epilogue_march": 0}, {"fused_epilogue": 0}])
def test_linear_family_as_functions_equals_linear_field_flux(ocn, arch, stepper, path):
    """the conditions of tests/test_gpu_parity.py:894-895 written as functions: every field == the LinearFieldFlux model after 3 steps, on
    the marching epilogue, the per-value epilogue and the stand-alone kernels"""
    F, rate = ocn.FieldBoundaryConditions, 2.5e-3
    common = {"u": F(top=ocn.FluxBoundaryCondition(-1e-3)), "T": F(top=ocn.FluxBoundaryCondition(4e-3), bottom=ocn.GradientBoundaryCondition(0.01))}
    linear = {"S": F(top=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(a=1e-4, b=-rate), field_dependencies="S"),
                     bottom=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(b=rate), field_dependencies="T"))}
    function = {"S": F(top=ocn.FluxBoundaryCondition(lambda x, y, t, S: 1e-4 + (-rate) * S, field_dependencies="S"),
                       bottom=ocn.FluxBoundaryCondition(lambda x, y, t, T, p: p * T, field_dependencies="T", parameters=rate))}
    out = []
    for bcs in (linear, function):
        grid = _grid(ocn, arch, "A")
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.ScalarDiffusivity(ν=1e-3, κ=2e-3), timestepper=stepper,
                                        boundary_conditions=common | bcs)
        for key, value in path.items():
            model.set_option(key, value)
        assert model.get_option("boundary_functions") == (2 if bcs is function else 0)
        ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=5))
        out.append(_run(ocn, model, 3, 0.05 * grid.Δxᶜᵃᵃ))
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n
    assert np.abs(out[0]["S"]).max() > 1 and np.isfinite(out[0]["S"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. drag: field-dependent and nonlinear
# ---------------------------------------------------------------------------------------------------------------------
class DragParameters:
    cD, V = 2.5e-3, 0.1


@pytest.mark.parametrize("which", ["A", "C"])
def test_quadratic_drag_equals_a_twin_fed_by_the_restatement(ocn, arch, which):
    """drag_u / drag_v of examples/tilted_bottom_boundary_layer.jl:122-126 on the bottom of u and v (AB2, ScalarDiffusivity): a twin carries
    array-valued Flux conditions that the test overwrites before every step with the restatement on the twin's own fields; 4 steps, =="""
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import boundary_functions as BF
    F, p = ocn.FieldBoundaryConditions, DragParameters()
    if which == "A":
        drag_u = lambda x, y, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * u                  # noqa: E731
        drag_v = lambda x, y, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * (v + p.V)          # noqa: E731
    else:                                                                                                # y is Flat: its coordinate is dropped
        drag_u = lambda x, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * u                     # noqa: E731
        drag_v = lambda x, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * (v + p.V)             # noqa: E731
    drags = {"u": drag_u, "v": drag_v}
    grid, twin_grid = _grid(ocn, arch, which), _grid(ocn, arch, which)
    shape = (grid.Nx, grid.Ny)
    kw = dict(tracers=("T",), closure=ocn.ScalarDiffusivity(ν=1e-3, κ=1e-3), timestepper="QuasiAdamsBashforth2")
    model = ocn.NonhydrostaticModel(grid=grid, boundary_conditions={n: F(bottom=ocn.FluxBoundaryCondition(f, field_dependencies=("u", "v"), parameters=p))
                                                                    for n, f in drags.items()}, **kw)
    arrays = {n: ocn.FluxBoundaryCondition(np.zeros(shape)) for n in drags}
    twin = ocn.NonhydrostaticModel(grid=twin_grid, boundary_conditions={n: F(bottom=bc) for n, bc in arrays.items()}, **kw)
    assert model.get_option("boundary_functions") == 2 and model.get_option("boundary_functions_read_time") == 0
    assert twin.get_option("boundary_functions") == 0 and twin.get_option("boundary_function_launches") == 0
    state = smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=3)
    state["v"] = state["v"] + 0.05
    ocn.set_model(model, **state)
    ocn.set_model(twin, **state)
    dt, last = 0.05 * grid.Δxᶜᵃᵃ, {}
    for _ in range(4):
        parents = {n: twin.fields()[n].parent() for n in ("u", "v")}
        for n, f in drags.items():
            last[n] = R.evaluate(f, twin_grid, BF.assumed_field_location(n), 4, [(parents[d], BF.assumed_field_location(d)) for d in ("u", "v")], twin.clock.time, p)
            _lib.check(_lib.lib().ocn_memcpy_h2d(arrays[n].device_array(shape), last[n].ctypes.data, last[n].nbytes))
        ocn.time_step(model, dt)
        ocn.time_step(twin, dt)
    for n, f in model.fields().items():
        assert np.array_equal(f.parent(), twin.fields()[n].parent()), n
    for n in drags:
        assert np.array_equal(model.boundary_function_values(n, "bottom"), last[n]), n
        assert np.abs(last[n]).max() > 1e-6
    model.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. stage times
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_substep", [1, 0])
def test_time_dependent_flux_sees_the_rk3_stage_times(ocn, arch, fuse_substep):
    """Q(t) = c t on top of a uniform tracer at rest: after one RK3 step from t₀ the top cells hold the three stage fluxes at t₀, t₀ + γ¹Δt and
    t₀ + (γ¹ + γ² + ζ²)Δt (runge_kutta_3.jl:93-170), everything below is unchanged to the bit, and the step is never replayed from a graph"""
    from oldoceananigans_jl_amd import _lib
    grid = _grid(ocn, arch, "B")
    c, t0, T0, dt = 0.3, 2.5, 1.0, 0.01
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",),
                                    boundary_conditions={"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(lambda x, y, t: c * t))})
    model.set_option("fuse_substep", fuse_substep)
    model.set_option("use_graph", 1)
    assert model.get_option("boundary_functions_read_time") == 1 and model.get_option("boundary_function_launches") == 1
    assert model.get_option("fuse_substep_active") == fuse_substep
    ocn.set_model(model, T=T0)
    _lib.check(_lib.lib().ocn_model_set_clock(model.handle, t0, 0, 1, float("inf"), float("inf")))
    ocn.time_step(model, dt)
    g1, g2, g3, z2, z3 = 8 / 15, 5 / 12, 3 / 4, -17 / 60, -5 / 12
    dz = grid.Δzᵃᵃᶜ[grid.Hz + grid.Nz - 1]
    times = (t0, t0 + dt * g1, (t0 + dt * g1) + dt * (g2 + z2))                                  # tick!(clock, γ¹Δt), tick!(clock, (γ² + ζ²)Δt)
    G = [-(c * t) / dz for t in times]                                                            # G[Nz] -= flux Az / V
    expected = T0 + dt * g1 * G[0]
    expected = expected + dt * (g2 * G[1] + z2 * G[0])
    expected = expected + dt * (g3 * G[2] + z3 * G[1])
    T = model.tracers.T.interior()
    print("top cells:", T[0, 0, -1], "expected", expected, "relative difference", abs(T[0, 0, -1] - expected) / abs(expected))
    assert np.all(np.abs(T[:, :, -1] - expected) <= 1e-14 * abs(expected))
    assert abs(expected - T0) > 1e-4                                  # (the three fluxes did something)
    assert np.all(T[:, :, :-1] == T0)
    assert np.array_equal(model.boundary_function_values("T", "top"), np.full((grid.Nx, grid.Ny), c * times[2]))
    for _ in range(5):
        ocn.time_step(model, dt)
    assert model.get_option("graph_replays") == 0 and model.get_option("graph_captures") == 0
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. graph
# ---------------------------------------------------------------------------------------------------------------------
def _drag_model(ocn, grid, functions=True, **kw):
    F, p = ocn.FieldBoundaryConditions, DragParameters()
    drag_u = lambda x, y, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * u                      # noqa: E731
    drag_v = lambda x, y, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + (v + p.V) ** 2) * (v + p.V)              # noqa: E731
    bcs = {"u": F(bottom=ocn.FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=p) if functions else ocn.FluxBoundaryCondition(-1e-4)),
           "v": F(bottom=ocn.FluxBoundaryCondition(drag_v, field_dependencies=("u", "v"), parameters=p) if functions else ocn.FluxBoundaryCondition(2e-4))}
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T",), closure=ocn.ScalarDiffusivity(ν=1e-3, κ=1e-3), boundary_conditions=bcs, **kw)
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=9))
    return model


def test_time_free_functions_keep_the_captured_step(ocn, arch):
    out = []
    for use_graph in (1, 0):
        grid = _grid(ocn, arch, "B")
        model = _drag_model(ocn, grid)
        model.set_option("use_graph", use_graph)
        out.append(_run(ocn, model, 6, 0.02 * grid.Δxᶜᵃᵃ))
        assert (model.get_option("graph_replays") > 0) == bool(use_graph)
        model.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


# ---------------------------------------------------------------------------------------------------------------------
# 6. replacement and accounting
# ---------------------------------------------------------------------------------------------------------------------
def test_replacement_and_accounting(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    grid, plain_grid = _grid(ocn, arch, "B"), _grid(ocn, arch, "B")
    model, plain = _drag_model(ocn, grid), _drag_model(ocn, plain_grid, functions=False)
    count = lambda m: (m.get_option("boundary_functions"), m.get_option("boundary_function_launches"))      # noqa: E731
    assert count(model) == (2, 1) and count(plain) == (0, 0)
    assert L.ocn_model_boundary_function_values(plain.handle, b"u", 4, np.zeros(1).ctypes.data_as(C.POINTER(C.c_double))) == -1
    _lib.check(L.ocn_model_set_boundary_condition(model.handle, b"u", 4, 1, -1e-4))
    assert count(model) == (1, 1)
    _lib.check(L.ocn_model_set_boundary_condition(model.handle, b"v", 4, 1, 2e-4))
    assert count(model) == (0, 0)
    dt = 0.02 * grid.Δxᶜᵃᵃ
    a, b = _run(ocn, model, 2, dt), _run(ocn, plain, 2, dt)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
    # a function replaces a function in place, the linear family replaces a function, unknown names are refused
    from oldoceananigans_jl_amd.boundary_functions import OPS, program_array
    prog, n = program_array([(OPS["field"], 0, 0, 0, 0.0)])
    deps = (C.c_char_p * 1)(b"u")
    for _ in range(2):
        _lib.check(L.ocn_model_set_flux_bc_function(model.handle, b"c0", 5, prog, n, deps, 1))
    assert count(model) == (1, 1)
    _lib.check(L.ocn_model_set_linear_flux_bc(model.handle, b"c0", 5, 0.0, 1.0, b"c0"))
    assert count(model) == (0, 0)
    assert L.ocn_model_set_flux_bc_function(model.handle, b"c0", 5, prog, n, (C.c_char_p * 1)(b"q"), 1) == -1
    assert L.ocn_model_set_flux_bc_function(model.handle, b"c7", 5, prog, n, deps, 1) == -1
    assert L.ocn_model_set_flux_bc_function(model.handle, b"w", 5, prog, n, deps, 1) == -1             # no Flux condition on w's own wall
    assert L.ocn_model_set_flux_bc_function(model.handle, b"c0", 5, prog, 0, deps, 1) == -1
    assert count(model) == (0, 0)
    model.close()
    plain.close()


def test_partitioned_models_refuse_functions(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import distributed as dist
    from oldoceananigans_jl_amd.boundary_functions import OPS, program_array
    L = _lib.lib()
    uid = C.create_string_buffer(128)
    _lib.check(L.ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    grid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    part = dist.LibraryDistributedModel(grid=grid, tracers=("T",))
    prog, n = program_array([(OPS["const"], 0, 0, 0, 1.0)])
    assert L.ocn_model_set_flux_bc_function(part.handle, b"c0", 5, prog, n, None, 0) == -2 and b"partitioned" in L.ocn_last_error()
    assert part.get_option("boundary_functions") == 0
    with pytest.raises(NotImplementedError, match="partitioned"):
        dist.LibraryDistributedModel(grid=grid, tracers=("T",),
                                     boundary_conditions={"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(lambda x, y, t: 1.0))})
    part.close()
    ctx.close()
