"""CPU tests of Relaxation with function masks and targets (forcings.py, boundary_functions.py; reference relaxation.jl:23-31, 80-101): the
recorded program instruction by instruction, the numpy interpreter against the user's own functions, the library's split of a program
(ocn_forcing_function_plan, host arithmetic only) against its restatement, the untouched built-in path and the refusals. No device."""
import ctypes as C

import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import boundary_functions as BF
from oldoceananigans_jl_amd import forcings as F

import forcing_function_reference as R
from helpers import tanh_faces

LOCS = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face),
        "T": (ocn.Center, ocn.Center, ocn.Center)}
OP = BF.OPS


def _grid(topology=(ocn.Bounded, ocn.Periodic, ocn.Bounded), size=(7, 5, 6)):
    kw = dict(x=(0.0, 2.0), y=(-1.0, 1.0), z=tanh_faces(size[-1]))
    kw = {d: kw[d] for d, t in zip("xyz", topology) if t is not ocn.Flat}
    return ocn.RectilinearGrid(None, size=tuple(n for n, t in zip(size, topology) if t is not ocn.Flat), topology=topology, **kw)


def _term(grid, name, relaxation):
    (t,) = F.model_forcing(grid, LOCS, {name: relaxation})[name]
    return t


def _ins(program):
    return [(BF.OP_NAMES[op], a, b, c, imm) for op, a, b, c, imm in program]


def test_a_function_mask_gives_a_function_term():
    """the capability itself: today's code refuses the callable"""
    grid = _grid()
    t = _term(grid, "T", ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x * z))
    assert t.kind == 3 and t.dep_names == ("T",) and not any(i[0] == OP["time"] for i in t.program)
    # rate * mask(x, y, z) first, then (0.0 - φ), then the product; leaves are emitted when first used
    assert _ins(t.program) == [("coord", 0, 0, 0, 0.0), ("coord", 2, 0, 0, 0.0), ("*", 0, 1, 0, 0.0), ("const", 0, 0, 0, 1.0), ("*", 3, 2, 0, 0.0),
                               ("const", 0, 0, 0, 0.0), ("field", 0, 0, 0, 0.0), ("-", 5, 6, 0, 0.0), ("*", 4, 7, 0, 0.0)]


def test_trace_of_a_callable_relaxation():
    grid = _grid()
    # a Number target is a constant; onefunction leaves the rate alone: rate * (target - φ)
    t = _term(grid, "u", ocn.Relaxation(rate=0.5, target=lambda x, y, z, t: t))
    assert _ins(t.program) == [("time", 0, 0, 0, 0.0), ("field", 0, 0, 0, 0.0), ("-", 0, 1, 0, 0.0), ("const", 0, 0, 0, 0.5), ("*", 3, 2, 0, 0.0)]
    assert t.dep_names == ("u",)
    t = _term(grid, "T", ocn.Relaxation(rate=2, mask=lambda x, y, z: z, target=3))
    assert _ins(t.program) == [("const", 0, 0, 0, 2.0), ("coord", 2, 0, 0, 0.0), ("*", 0, 1, 0, 0.0), ("const", 0, 0, 0, 3.0), ("field", 0, 0, 0, 0.0),
                               ("-", 3, 4, 0, 0.0), ("*", 2, 5, 0, 0.0)]
    # zerofunction: 0.0 - φ
    t = _term(grid, "T", ocn.Relaxation(rate=2.0, mask=lambda x, y, z: y))
    assert _ins(t.program)[3:] == [("const", 0, 0, 0, 0.0), ("field", 0, 0, 0, 0.0), ("-", 3, 4, 0, 0.0), ("*", 2, 5, 0, 0.0)]
    # built-ins next to a function are recorded by their reference formulas
    t = _term(grid, "T", ocn.Relaxation(rate=0.25, mask=ocn.GaussianMask("z", center=-0.5, width=0.2), target=lambda x, y, z, t: x))
    assert _ins(t.program) == [("coord", 2, 0, 0, 0.0), ("const", 0, 0, 0, -0.5), ("-", 0, 1, 0, 0.0), ("*", 2, 2, 0, 0.0), ("neg", 3, 0, 0, 0.0),
                               ("const", 0, 0, 0, 2 * (0.2 * 0.2)), ("/", 4, 5, 0, 0.0), ("exp", 6, 0, 0, 0.0), ("const", 0, 0, 0, 0.25),
                               ("*", 8, 7, 0, 0.0), ("coord", 0, 0, 0, 0.0), ("field", 0, 0, 0, 0.0), ("-", 10, 11, 0, 0.0), ("*", 9, 12, 0, 0.0)]
    t = _term(grid, "T", ocn.Relaxation(rate=1.0, mask=ocn.PiecewiseLinearMask("x", center=1.0, width=0.5),
                                        target=lambda x, y, z, t: t))
    names = [i[0] for i in _ins(t.program)]
    assert names[:9] == ["coord", "const", "-", "abs", "const", "/", "const", "-", "const"] and names[9] == "max"
    t = _term(grid, "T", ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x, target=ocn.LinearTarget("y", intercept=1.5, gradient=2.0)))
    assert _ins(t.program)[3:8] == [("const", 0, 0, 0, 2.0), ("coord", 1, 0, 0, 0.0), ("*", 3, 4, 0, 0.0), ("const", 0, 0, 0, 1.5), ("+", 6, 5, 0, 0.0)]


@pytest.mark.parametrize("topology,arguments", [((ocn.Periodic, ocn.Flat, ocn.Bounded), "xz"), ((ocn.Flat, ocn.Periodic, ocn.Bounded), "yz"),
                                                ((ocn.Periodic, ocn.Periodic, ocn.Flat), "xy"), ((ocn.Flat, ocn.Flat, ocn.Bounded), "z")])
def test_signature_drops_flat_directions(topology, arguments):
    """mask(X...) and target(X..., t) with X the non-Flat node coordinates; OCN_EXPR_COORD still names x / y / z absolutely"""
    grid = _grid(topology)
    seen = {}

    def mask(*X):
        seen["mask"] = len(X)
        return X[-1]

    def target(*Xt):
        seen["target"] = len(Xt)
        return Xt[0] + Xt[-1]

    t = _term(grid, "T", ocn.Relaxation(rate=1.0, mask=mask, target=target))
    assert seen == {"mask": len(arguments), "target": len(arguments) + 1}
    coords = [i[1] for i in _ins(t.program) if i[0] == "coord"]
    assert coords == ["xyz".index(arguments[-1]), "xyz".index(arguments[0])][:len(set(arguments[-1] + arguments[0]))]
    # a built-in along the Flat direction stays the ValueError it is without a function
    flat = "xyz"[[q for q in range(3) if topology[q] is ocn.Flat][0]]
    with pytest.raises(ValueError, match="Flat"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask(flat, center=0.0, width=1.0), target=target))
    with pytest.raises(ValueError, match="Flat"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask=mask, target=ocn.LinearTarget(flat, intercept=0.0, gradient=1.0)))


def test_numpy_interpreter_equals_the_functions():
    """forcings.evaluate on the recorded program == rate * mask(X...) * (target(X..., t) - φ) with the user's functions on numpy arrays"""
    rng = np.random.default_rng(3)
    for topology in ((ocn.Bounded, ocn.Periodic, ocn.Bounded), (ocn.Periodic, ocn.Flat, ocn.Bounded)):
        grid = _grid(topology)
        flat = topology[1] is ocn.Flat
        mask = (lambda x, z: ocn.max_(1.0 - abs(x - 0.5) / 0.75, ocn.exp(-(z + 0.25) ** 2 / 0.1))) if flat else \
               (lambda x, y, z: ocn.max_(1.0 - abs(x - 0.5) / 0.75, ocn.exp(-(z + 0.25) ** 2 / 0.1)) * (1.0 + y))
        target = (lambda x, z, t: ocn.tanh(z / 0.3) + ocn.sin(2.0 * t) * x) if flat else (lambda x, y, z, t: ocn.tanh(z / 0.3) + ocn.sin(2.0 * t) * x)
        for name, loc in LOCS.items():
            terms = F.model_forcing(grid, LOCS, {name: ocn.Relaxation(rate=0.7, mask=mask, target=target)})[name]
            phi = rng.standard_normal(grid.interior_size(loc))
            X = R.coordinates(grid, loc)
            want = 0.7 * mask(*X) * (target(*X, 1.25) - phi)
            got = F.evaluate(terms, grid, loc, phi, t=1.25)
            assert got.shape == want.shape == tuple(grid.interior_size(loc)) and np.array_equal(got, want), (name, flat)


def _plan(program, ndeps=1):
    from oldoceananigans_jl_amd import _lib
    arr, n = BF.program_array(program)
    cls, n_cell = (C.c_int * max(n, 1))(), C.c_int(-1)
    status = _lib.lib().ocn_forcing_function_plan(arr, n, ndeps, cls, C.byref(n_cell))
    return status, list(cls)[:n], n_cell.value


def _random_function(rng, nops):
    """a random function of (x, y, z, t, φ): every operation draws its operands from the values so far"""
    unary = [lambda a: -a, abs, ocn.exp, ocn.tanh, lambda a: a ** 2]
    binary = [lambda a, b: a + b, lambda a, b: a - b, lambda a, b: a * b, ocn.min_, ocn.max_, lambda a, b: ocn.ifelse(a > b, a, b)]
    choices = rng.integers(0, 1 << 30, size=(nops, 4))

    def f(x, y, z, t, phi):
        pool = [x, y, z, t, phi, 0.5]
        # programs that mix classes: a few values of one coordinate first, the field late
        values = [pool[c % 3] for c in choices[:3, 0]] + [t, 1.5]
        for q, (kind, i, j, k) in enumerate(choices):
            source = values + ([phi] if q > nops // 2 else []) + ([pool[k % 3]] if k % 4 == 0 else [])
            a, b = source[i % len(source)], source[j % len(source)]
            values.append(unary[k % len(unary)](a) if kind % 3 == 0 else binary[k % len(binary)](a, b))
        return values[-1]
    return f


def test_plan_equals_the_restatement():
    """the class of every value and the per-cell length, from the library's host code, == tests/forcing_function_reference.py"""
    grid = _grid()
    sponge = _term(grid, "T", ocn.Relaxation(rate=1 / 60, mask=lambda x, y, z: ocn.exp(-(z + 0.8) ** 2 / (2 * 0.1 ** 2)),
                                             target=lambda x, y, z, t: 20.0 + 0.01 * z + 0.5 * ocn.sin(0.1 * t))).program
    status, cls, n_cell = _plan(sponge)
    assert status == 0 and cls == R.value_classes(sponge) and n_cell == R.cell_length(sponge)
    # two table loads, the field, a subtraction and a multiplication: what forcing_one does
    assert n_cell == 5 and set(cls) == {R.UNIFORM, R.LINE_Z, R.CELL} and cls.count(R.CELL) == 3
    product = _term(grid, "T", ocn.Relaxation(rate=2.0, mask=lambda x, y, z: (1.0 + x * x) * ocn.exp(z))).program
    status, cls, n_cell = _plan(product)
    assert status == 0 and cls == R.value_classes(product) and n_cell == R.cell_length(product)
    assert {R.LINE_X, R.LINE_Z} <= set(cls)
    mixed = _term(grid, "T", ocn.Relaxation(rate=2.0, mask=lambda x, y, z: ocn.exp(-(x ** 2 + z ** 2)))).program
    status, cls, n_cell = _plan(mixed)
    assert status == 0 and cls == R.value_classes(mixed) and n_cell == R.cell_length(mixed)
    assert cls[[i[0] for i in _ins(mixed)].index("exp")] == R.CELL
    line = BF.trace(lambda x, y, z, t, phi: 0.0 * t + ocn.tanh(z / 0.3), [0, 1, 2], 1)            # the result is a line value
    status, cls, n_cell = _plan(line)
    assert status == 0 and cls == R.value_classes(line) and cls[-1] == R.LINE_Z and n_cell == R.cell_length(line) == 1
    rng = np.random.default_rng(20)
    kinds = set()
    for q in range(20):
        program = BF.trace(_random_function(rng, int(rng.integers(4, 40))), [0, 1, 2], 1)
        status, cls, n_cell = _plan(program)
        assert status == 0 and cls == R.value_classes(program) and n_cell == R.cell_length(program), q
        kinds |= set(cls)
    assert kinds == {R.UNIFORM, R.LINE_X, R.LINE_Y, R.LINE_Z, R.CELL}


def test_plan_refuses_bad_programs():
    good = [(OP["coord"], 2, 0, 0, 0.0), (OP["field"], 0, 0, 0, 0.0), (OP["*"], 0, 1, 0, 0.0)]
    assert _plan(good)[0] == 0
    assert _plan([(OP["coord"], 3, 0, 0, 0.0)])[0] != 0                       # x / y / z are 0 / 1 / 2
    assert _plan(good, ndeps=0)[0] != 0                                       # dependency slot 0 of none
    assert _plan([(OP["*"], 0, 0, 0, 0.0)])[0] != 0                           # an operand that is no earlier value
    assert _plan([(99, 0, 0, 0, 0.0)])[0] != 0
    assert _plan([(24, 0, 0, 0, 0.0)])[0] != 0                                # the library's table load is not a public op
    assert _plan(good * 22)[0] != 0                                           # 66 instructions


def test_built_in_relaxations_are_unchanged():
    """no function: kind 2 with the host tables, bit for bit what `rate * mask(node)` and `target(node)` give"""
    grid = _grid()
    nodes = {("z", ocn.Face): grid.zᵃᵃᶠ, ("z", ocn.Center): grid.zᵃᵃᶜ}
    for name, loc in LOCS.items():
        mask, target = ocn.GaussianMask("z", center=-0.5, width=0.3), ocn.LinearTarget("z", intercept=2, gradient=0.5)
        t = _term(grid, name, ocn.Relaxation(rate=1 / 7, mask=mask, target=target))
        xi = np.asarray(nodes[("z", loc[2])])
        assert t.kind == 2 and t.program is None and (t.mask_dir, t.target_dir) == (2, 2)
        assert np.array_equal(t.mask_table, (1 / 7) * np.exp(-((xi + 0.5) * (xi + 0.5)) / (2 * (0.3 * 0.3))))
        assert np.array_equal(t.target_table, 2.0 + 0.5 * xi)
    for r in (ocn.Relaxation(rate=2.0), ocn.Relaxation(rate=2.0, target=1.5), ocn.Relaxation(rate=1.0, mask=F.onefunction, target=F.zerofunction),
              ocn.Relaxation(rate=1.0, mask=ocn.PiecewiseLinearMask("x", center=1.0, width=0.5))):
        assert _term(grid, "T", r).kind == 2
    terms = F.model_forcing(grid, LOCS, {"T": (ocn.Relaxation(rate=1.0), ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x))})["T"]
    assert [t.kind for t in terms] == [2, 3]


def test_limits_and_refusals():
    grid = _grid()

    def long_mask(x, y, z):
        for _ in range(70):
            x = x + 1.0
        return x
    with pytest.raises(ValueError, match="64"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask=long_mask))
    with pytest.raises(TypeError, match="ocn.ifelse"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x if x > 0 else z))
    with pytest.raises(TypeError):
        _term(grid, "T", ocn.Relaxation(rate=1.0, target=lambda x, y, z, t: "warm"))
    with pytest.raises(NotImplementedError, match="Relaxation"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask="everywhere", target=lambda x, y, z, t: t))
    with pytest.raises(NotImplementedError, match="Relaxation"):
        _term(grid, "T", ocn.Relaxation(rate=1.0, mask="everywhere"))
    # eight dependencies per program (a relaxation has one; the raw evaluation takes any number up to the limit)
    BF.trace(lambda x, y, z, t, *deps: deps[0] + deps[7], [0, 1, 2], 8)
    with pytest.raises(ValueError, match="8"):
        BF.trace(lambda x, y, z, t, *deps: deps[0], [0, 1, 2], 9)
    assert _plan([(OP["const"], 0, 0, 0, 1.0)], ndeps=8)[0] == 0 and _plan([(OP["const"], 0, 0, 0, 1.0)], ndeps=9)[0] != 0
    # sixteen function terms per model
    sponge = ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x)
    F.model_forcing(grid, LOCS, {n: (sponge,) * 4 for n in LOCS})
    with pytest.raises(ValueError, match="16"):
        F.model_forcing(grid, LOCS, {"u": (sponge,) * 8, "v": (sponge,) * 8, "T": sponge})
    # the pinned refusals keep their words
    with pytest.raises(NotImplementedError, match="callable"):
        F.model_forcing(grid, LOCS, {"T": lambda x, y, z, t: 1.0})
    with pytest.raises(NotImplementedError, match="ContinuousForcing"):
        F.model_forcing(grid, LOCS, {"T": ocn.Forcing(lambda x, y, z, t: 1.0)})


def test_partitioned_grids_are_refused_before_any_handle():
    class Partitioned:
        local = _grid()
    terms = F.model_forcing(Partitioned.local, LOCS, {"T": ocn.Relaxation(rate=1.0, mask=lambda x, y, z: x)})
    with pytest.raises(NotImplementedError, match="partitioned"):
        F.refuse_functions_on_partitions(terms, Partitioned())
    F.refuse_functions_on_partitions(terms, Partitioned.local)
    built_in = F.model_forcing(Partitioned.local, LOCS, {"T": ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask("x", center=0.0, width=1.0))})
    F.refuse_functions_on_partitions(built_in, Partitioned())            # the built-in path on partitions is untouched
