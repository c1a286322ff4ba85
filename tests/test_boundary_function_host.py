"""Host side of FluxBoundaryCondition(func, field_dependencies, parameters) (no device): the recorded program of a function, its
agreement with the function itself through the numpy interpreter of tests/boundary_function_reference.py, the call signature, the
interpolation operators, the limits and the refusals."""
import numpy as np
import pytest

import boundary_function_reference as R

from oldoceananigans_jl_amd import boundary_functions as BF

OP = BF.OPS


def _names(program):
    return [(BF.OP_NAMES[op], a, b, c, imm) for op, a, b, c, imm in program]


def test_trace_of_the_quadratic_drag_in_evaluation_order():
    import oldoceananigans_jl_amd as ocn
    cD, V = 2e-3, 0.1
    program = BF.trace(lambda x, y, t, u, v: -cD * ocn.sqrt(u ** 2 + (v + V) ** 2) * u, [0, 1], 2)
    assert _names(program) == [("field", 0, 0, 0, 0.0), ("*", 0, 0, 0, 0.0),                       # u ** 2: u * u
                               ("field", 1, 0, 0, 0.0), ("const", 0, 0, 0, V), ("+", 2, 3, 0, 0.0),      # v + V
                               ("*", 4, 4, 0, 0.0), ("+", 1, 5, 0, 0.0), ("sqrt", 6, 0, 0, 0.0),
                               ("const", 0, 0, 0, -cD), ("*", 8, 7, 0, 0.0), ("*", 9, 0, 0, 0.0)]        # -cD is Python's; the last value is the flux


def test_powers_constants_sharing_and_plain_numbers():
    import oldoceananigans_jl_amd as ocn
    assert [n[0] for n in _names(BF.trace(lambda t, u: u ** 2, [], 1))] == ["field", "*"]
    assert _names(BF.trace(lambda t, u: u ** 3, [], 1)) == [("field", 0, 0, 0, 0.0), ("*", 0, 0, 0, 0.0), ("*", 1, 0, 0, 0.0)]
    assert [n[0] for n in _names(BF.trace(lambda t, u: u ** 2.5, [], 1))] == ["field", "const", "pow"]
    assert [n[0] for n in _names(BF.trace(lambda t, u, v: u ** v, [], 2))] == ["field", "field", "pow"]
    assert [n[0] for n in _names(BF.trace(lambda t, u: 2.0 ** u, [], 1))] == ["const", "field", "pow"]
    # 2 * 3 is Python's (6.0); u * 2 * 3 is two multiplications: nothing is folded or reassociated, and * 1 stays
    assert _names(BF.trace(lambda t, u: 2 * 3 * u, [], 1)) == [("const", 0, 0, 0, 6.0), ("field", 0, 0, 0, 0.0), ("*", 0, 1, 0, 0.0)]
    assert [n[0] for n in _names(BF.trace(lambda t, u: u * 2 * 3, [], 1))] == ["field", "const", "*", "const", "*"]
    assert [n[0] for n in _names(BF.trace(lambda t, u: u * 1, [], 1))] == ["field", "const", "*"]

    def shared(t, u, v):
        s = ocn.sqrt(u * u + v * v)
        return s * u + s * v                                                  # s is one Python object: emitted once
    assert [n[0] for n in _names(BF.trace(shared, [], 2))].count("sqrt") == 1
    assert [n[0] for n in _names(BF.trace(lambda t, u: ocn.sqrt(u) + ocn.sqrt(u), [], 1))].count("sqrt") == 2
    # a plain number: one instruction; a bare argument: its leaf; an earlier value returned: copied to the end exactly (max(x, x))
    assert BF.trace(lambda x, y, t: 4, [0, 1], 0) == [(OP["const"], 0, 0, 0, 4.0)]
    assert BF.trace(lambda x, y, t: y, [0, 1], 0) == [(OP["coord"], 1, 0, 0, 0.0)]
    assert BF.trace(lambda x, t: t, [1], 0) == [(OP["time"], 0, 0, 0, 0.0)]

    def earlier(t, u):
        a = u + 1
        a * 2
        return a
    assert [n[0] for n in _names(BF.trace(earlier, [], 1))][-1] == "max"
    # every other operation: one instruction each
    f = lambda t, u, v: ocn.ifelse(u < v, -u, abs(v)) + ocn.min_(u, v) - ocn.max_(u, 2) / ocn.exp(ocn.log(ocn.sin(ocn.cos(ocn.tanh(u)))))   # noqa: E731
    ops = [n[0] for n in _names(BF.trace(f, [], 2))]
    for name in ("<", "neg", "abs", "select", "min", "max", "exp", "log", "sin", "cos", "tanh", "+", "-", "/"):
        assert ops.count(name) == 1, name
    assert [n[0] for n in _names(BF.trace(lambda t, u: ocn.ifelse(u >= 0, 1.0, ocn.ifelse(u <= -1, 2.0, u > 3)), [], 1))].count("select") == 2
    # the new functions also work on plain numbers and arrays
    assert ocn.sqrt(4.0) == 2.0 and ocn.exp(0.0) == 1.0 and ocn.log(1.0) == 0.0 and ocn.sin(0.0) == 0.0 and ocn.cos(0.0) == 1.0 and ocn.tanh(0.0) == 0.0
    assert ocn.ifelse(True, 1.0, 2.0) == 1.0 and ocn.min_(1.0, 2.0) == 1.0 and ocn.max_(1.0, 2.0) == 2.0
    assert np.array_equal(ocn.ifelse(np.array([1.0, -1.0]) > 0, 5.0, np.array([7.0, 8.0])), [5.0, 8.0])


def test_control_flow_on_a_symbol_and_the_limits():
    import oldoceananigans_jl_amd as ocn
    with pytest.raises(TypeError, match="ocn.ifelse"):
        BF.trace(lambda t, u: 1.0 if u > 0 else 2.0, [], 1)
    with pytest.raises(TypeError, match="ocn.ifelse"):
        BF.trace(lambda t, u: min(u, 1.0), [], 1)
    with pytest.raises(TypeError):
        BF.trace(lambda t, u: "flux", [], 1)

    def long(t, u):
        for _ in range(64):
            u = u + 1.0
        return u
    with pytest.raises(ValueError, match="64"):
        BF.trace(long, [], 1)

    def fits(t, u):                                      # the leaf + 31 x (constant, addition) = 63 instructions
        for _ in range(31):
            u = u + 1.0
        return u
    assert len(BF.trace(fits, [], 1)) == 63
    with pytest.raises(ValueError, match="8"):
        ocn.FluxBoundaryCondition(lambda *a: 0.0, field_dependencies=("u", "v", "w", "T", "S", "u", "v", "w", "T"))
    assert len(ocn.FluxBoundaryCondition(lambda *a: 0.0, field_dependencies=("u",) * 8).function.field_dependencies) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the recorded program computes what the function computes
# ---------------------------------------------------------------------------------------------------------------------
def _random_function(rng, nargs, depth=3):
    """a random expression over + - * / abs min max sqrt ifelse of the arguments (coordinates, t, dependencies) and constants, as a
    function that works on symbols and on numpy arrays alike"""
    import oldoceananigans_jl_amd as ocn

    def build(d):
        if d == 0 or rng.random() < 0.15:
            if rng.random() < 0.3:
                c = float(rng.normal())
                return lambda args: c
            q = int(rng.integers(nargs))
            return lambda args: args[q]
        kind = rng.choice(["+", "-", "*", "/", "abs", "min", "max", "sqrt", "ifelse", "neg", "sq"])
        a, b, c = build(d - 1), build(d - 1), build(d - 1)
        return {"+": lambda args: a(args) + b(args), "-": lambda args: a(args) - b(args), "*": lambda args: a(args) * b(args),
                "/": lambda args: a(args) / b(args), "abs": lambda args: abs(a(args) + 0.5), "min": lambda args: ocn.min_(a(args), b(args)),
                "max": lambda args: ocn.max_(a(args), b(args)), "sqrt": lambda args: ocn.sqrt(abs(a(args) + 1.0)),
                "ifelse": lambda args: ocn.ifelse(a(args) + 0.1 < b(args), c(args) + 1.0, 2.0 - b(args)),
                "neg": lambda args: -(a(args) + 0.25), "sq": lambda args: (a(args) - 0.5) ** 2}[kind]
    tree = build(depth)
    return lambda *args: tree(args) + args[0] * 0.5                   # (always a symbol in the end)


def _grids(ocn):
    from helpers import tanh_faces
    B, P, F = ocn.Bounded, ocn.Periodic, ocn.Flat
    return [ocn.RectilinearGrid(None, size=(7, 5, 6), x=(0.0, 1.0), y=(-1.0, 1.0), z=tanh_faces(6), topology=(B, B, B)),
            ocn.RectilinearGrid(None, size=(6, 4), x=(0.0, 2.0), z=(-1.0, 0.0), topology=(B, F, B))]


LOCATIONS = ["u", "v", "w", "T"]


def test_interpreter_on_the_traced_program_equals_the_function():
    """randomised functions over all six sides and the four field locations: interpret(trace(f)) == f on the same arrays, bit for bit"""
    import oldoceananigans_jl_amd as ocn
    rng = np.random.default_rng(7)
    checked = 0
    for grid in _grids(ocn):
        parents = {n: rng.standard_normal(grid.total_size(BF.assumed_field_location(n))) for n in LOCATIONS}
        for side in range(6):
            if grid.topology[side // 2] is not ocn.Bounded:
                continue
            for name in LOCATIONS:
                loc = BF.assumed_field_location(name)
                deps = ("u", "v", "w", "T")
                X, both = R.boundary_coordinates(grid, loc, side)
                func = _random_function(rng, len(X) + 1 + len(deps))
                rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(func, None, deps), grid, loc, side, deps)
                ta, tb = BF.tangential_directions(side)
                shape = (grid.size[ta], grid.size[tb])
                values = [R.dependency_at_boundary(grid, parents[d], BF.assumed_field_location(d), loc, side) for d in deps]
                with np.errstate(all="ignore"):
                    direct = R.evaluate(func, grid, loc, side, [(parents[d], BF.assumed_field_location(d)) for d in deps], 0.75)
                interpreted = R.interpret(rbf.program, both, 0.75, values, shape)
                assert np.array_equal(direct, interpreted, equal_nan=True), (grid.size, side, name)
                assert np.isfinite(direct).mean() > 0.5
                checked += 1
    assert checked == 6 * 4 + 4 * 4


def test_signature_follows_the_flat_directions_and_the_parameters():
    import oldoceananigans_jl_amd as ocn
    B, P, F = ocn.Bounded, ocn.Periodic, ocn.Flat
    seen = []

    def spy(*args):
        seen.append(args)
        return 0.0
    u_loc = BF.assumed_field_location("u")
    names = ("u", "v", "w", "T")
    for topology, size, kw, ncoords in (((P, P, B), (4, 4, 4), dict(x=(0, 1), y=(0, 1), z=(-1, 0)), 2),
                                        ((P, F, B), (4, 4), dict(x=(0, 1), z=(-1, 0)), 1),
                                        ((F, F, B), (4,), dict(z=(-1, 0)), 0)):
        grid = ocn.RectilinearGrid(None, size=size, topology=topology, **kw)
        for parameters in (None, {"cD": 1e-3}):
            seen.clear()
            rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(spy, parameters, ("u", "v")), grid, u_loc, 4, names)
            args = seen[0]
            assert len(args) == ncoords + 1 + 2 + (parameters is not None)                    # X..., t, u, v, [p]
            assert all(isinstance(a, BF.Symbol) for a in args[:ncoords + 3])
            assert [a.leaf[0] for a in args[:ncoords + 3]] == ["coord"] * ncoords + ["time", "field", "field"]
            if parameters is not None:
                assert args[-1] is parameters
            assert len(rbf.coordinates) == ncoords
    # drag_u(x, t, u, v, p) of the tilted bottom boundary layer on (Periodic, Flat, Bounded): x is the FIRST tangential coordinate
    grid = ocn.RectilinearGrid(None, size=(4, 4), x=(0, 1), z=(-1, 0), topology=(P, F, B))
    rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(lambda x, t, u, v, p: x * p, 2.0, ("u", "v")), grid, u_loc, 4, names)
    assert rbf.program[0] == (OP["coord"], 0, 0, 0, 0.0) and not rbf.reads_time
    # on a west side of (Flat, Periodic, Bounded)... is no wall; on the south side of (Flat, Bounded, Bounded) the one coordinate is z: the SECOND
    grid = ocn.RectilinearGrid(None, size=(4, 4), y=(0, 1), z=(-1, 0), topology=(F, B, B))
    rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(lambda z, t: z * t, None, ()), grid, u_loc, 2, names)
    assert rbf.program[0] == (OP["coord"], 1, 0, 0, 0.0) and rbf.reads_time and rbf.location == (ocn.Face, None, ocn.Center)


def test_interpolation_operator_names_and_unknown_dependencies():
    import oldoceananigans_jl_amd as ocn
    B, P = ocn.Bounded, ocn.Periodic
    grid = ocn.RectilinearGrid(None, size=(4, 4, 4), extent=(1, 1, 1), topology=(P, P, B))
    names = ("u", "v", "w", "T", "S")
    rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(lambda x, y, t, u, v, w, T: u, None, ("u", "v", "w", "T")),
                                         grid, BF.assumed_field_location("u"), 4, names)
    assert rbf.interps == ("identity", "ℑxyᶠᶜᵃ", "ℑxᶠᵃᵃ", "ℑxᶠᵃᵃ")                 # never along the normal: w's z location does not count
    assert rbf.location == (ocn.Face, ocn.Center, None)
    rbf = BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(lambda x, y, t, u, v: v, None, ("u", "v")), grid,
                                         BF.assumed_field_location("T"), 5, names)
    assert rbf.interps == ("ℑxᶜᵃᵃ", "ℑyᵃᶜᵃ")
    with pytest.raises(ValueError) as e:
        BF.RegularizedBoundaryFunction(BF.ContinuousBoundaryFunction(lambda x, y, t, q: q, None, ("q",)), grid, BF.assumed_field_location("T"), 5, names)
    assert "('q',)" in str(e.value) and "'u', 'v', 'w', 'T', 'S'" in str(e.value)


def test_refusals_name_their_case():
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd.boundary_conditions import bc_table, validate_boundary_functions
    f = lambda x, y, t: 0.0                                                                     # noqa: E731
    bc = ocn.FluxBoundaryCondition(f)
    assert bc.function is not None and bc.classification == "Flux" and bc.array is None and "ContinuousBoundaryFunction" in repr(bc)
    assert ocn.FluxBoundaryCondition(f, field_dependencies="T", parameters=3.0).function.field_dependencies == ("T",)
    for make, word in ((ocn.ValueBoundaryCondition, "Value"), (ocn.GradientBoundaryCondition, "Gradient"), (ocn.OpenBoundaryCondition, "Open")):
        with pytest.raises(NotImplementedError, match=word):
            make(f)
    with pytest.raises(NotImplementedError, match="discrete_form"):
        ocn.FluxBoundaryCondition(lambda i, j, grid, clock, fields: 0.0, discrete_form=True)
    # the free-standing fill / flux computation has no clock and no model fields
    with pytest.raises(NotImplementedError, match="clock"):
        bc_table([ocn.FieldBoundaryConditions(top=bc)])
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    fbcs = ocn.FieldBoundaryConditions(top=bc)
    validate_boundary_functions({"T": fbcs, "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1.0))}, grid)

    class Partitioned:
        local, topology = grid, grid.topology
    with pytest.raises(NotImplementedError, match="partitioned"):
        validate_boundary_functions({"T": fbcs}, Partitioned())
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=Partitioned(), boundary_conditions={"T": fbcs})
    for name, entry in (("νₑ", fbcs), ("κₑ", {"T": fbcs})):
        with pytest.raises(NotImplementedError, match="diffusivity"):
            validate_boundary_functions({name: entry}, grid)
        with pytest.raises(NotImplementedError, match="diffusivity"):
            ocn.NonhydrostaticModel(grid=grid, closure=ocn.AnisotropicMinimumDissipation(), boundary_conditions={name: entry})


def test_callable_open_conditions_and_forcings_stay_refused():
    import oldoceananigans_jl_amd as ocn
    with pytest.raises(NotImplementedError):
        ocn.OpenBoundaryCondition(lambda y, z, t: 0.1 * t)
    with pytest.raises(NotImplementedError):
        ocn.OpenBoundaryCondition(lambda y, z, t: 0.1 * t, scheme=ocn.PerturbationAdvection())
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    with pytest.raises(NotImplementedError, match="callable"):
        ocn.NonhydrostaticModel(grid=grid, forcing={"u": lambda x, y, z, t: 0.0})
    with pytest.raises(NotImplementedError, match="ContinuousForcing"):
        ocn.NonhydrostaticModel(grid=grid, forcing={"u": ocn.Forcing(lambda x, y, z, t: 0.0)})
    with pytest.raises(NotImplementedError, match="AdvectiveForcing"):
        ocn.NonhydrostaticModel(grid=grid, forcing={"T": ocn.AdvectiveForcing(w=1.0)})
