"""CPU tests of stencil programs: what ocn.KernelFunctionOperation and the operators of ocn.operators record, the slot plan of the
library (host arithmetic, no device), the two routes of tests/stencil_reference.py against each other, the lowering of Derivative /
UnaryOperation / at, and every limit and refusal. Grids have architecture None and fields are borrowed: nothing touches a device."""
import ctypes as C

import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn
import stencil_reference as R
from helpers import tanh_faces
from oldoceananigans_jl_amd import diagnostics, operators as O

Ce, Fa = ocn.Center, ocn.Face
CCC, FCC, CFC, CCF, FFC = R.CCC, R.FCC, R.CFC, R.CCF, R.FFC
BPB = (ocn.Bounded, ocn.Periodic, ocn.Bounded)
OP = O.OPS


class Host:
    """a grid without a device, four borrowed fields and random host parents (halos included)"""

    def __init__(self, topology, size, **kw):
        self.grid = ocn.RectilinearGrid(None, size=size, topology=topology, **kw)
        rng = np.random.default_rng(11)
        self.f, self.p = {}, {}
        for n, loc in (("T", CCC), ("u", FCC), ("v", CFC), ("w", CCF)):
            self.f[n] = ocn.Field(loc, self.grid, data=C.c_void_p(0))
            self.p[n] = np.asfortranarray(0.5 + rng.standard_normal(self.f[n].shape))

    def parents(self, stencil):
        return [self.p[next(n for n, f in self.f.items() if f is g)] for g in stencil.fields]


GRIDS = {
    "bpb_stretched": lambda: Host(BPB, (70, 37, 9), x=(0, 1), y=(0, 1), z=tanh_faces(9)),
    "slice": lambda: Host((ocn.Bounded, ocn.Flat, ocn.Bounded), (66, 16), x=(0, 1), z=(-1, 0)),
    "ppp": lambda: Host((ocn.Periodic,) * 3, (16, 16, 16), x=(0, 1), y=(0, 1), z=(0, 1)),
    "halo_534": lambda: Host((ocn.Periodic, ocn.Periodic, ocn.Bounded), (12, 10, 8), x=(0, 1), y=(0, 1), z=tanh_faces(8), halo=(5, 3, 4)),
}


@pytest.fixture(scope="module")
def hosts():
    return {n: make() for n, make in GRIDS.items()}


def named(h, name):
    loc, fn, args = R.KERNEL_FUNCTIONS[name]
    return ocn.KernelFunctionOperation(loc, fn, h.grid, *[h.f[a] for a in args]), [h.p[a] for a in args]


# ---------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------
def test_trace_of_vorticity_instruction_by_instruction(hosts):
    h = hosts["ppp"]
    k = ocn.KernelFunctionOperation(FFC, O.ζ3ᶠᶠᶜ, h.grid, h.f["u"], h.f["v"])
    dx = dy = 1 / 16
    L, K, MUL, SUB = OP["load"], OP["const"], OP["*"], OP["-"]
    assert k.stencil.program == [
        (L, 1, 0, 0, 0, 0, 0, 0.0),                 # v[i, j, k]
        (K, 0, 0, 0, 0, 0, 0, dy),                  # Δyᶜᶠᶜ
        (MUL, 1, 0, 0, 0, 0, 0, 0.0),               # Δy_qᶜᶠᶜ at i
        (L, 1, 0, 0, -1, 0, 0, 0.0),                # v[i - 1, j, k]
        (MUL, 1, 3, 0, 0, 0, 0, 0.0),
        (SUB, 2, 4, 0, 0, 0, 0, 0.0),               # δxᶠᶠᶜ
        (L, 0, 0, 0, 0, 0, 0, 0.0),                 # u[i, j, k]; Δxᶠᶜᶜ has the bits of Δy here: ONE constant
        (MUL, 1, 6, 0, 0, 0, 0, 0.0),
        (L, 0, 0, 0, 0, -1, 0, 0.0),                # u[i, j - 1, k]
        (MUL, 1, 8, 0, 0, 0, 0, 0.0),
        (SUB, 7, 9, 0, 0, 0, 0, 0.0),               # δyᶠᶠᶜ
        (SUB, 5, 10, 0, 0, 0, 0, 0.0),              # Γᶠᶠᶜ
        (K, 0, 0, 0, 0, 0, 0, 1 / (dx * dy)),       # Az⁻¹ᶠᶠᶜ = 1 / (Δx Δy), formed by the host
        (MUL, 11, 12, 0, 0, 0, 0, 0.0)]
    assert [f is g for f, g in zip(k.stencil.fields, (h.f["u"], h.f["v"]))] == [True, True]
    text = repr(k)
    assert text.startswith("KernelFunctionOperation at (Face, Face, Center)\n├── grid: 16×16×16 RectilinearGrid")
    assert "├── kernel_function: " in text and text.endswith('└── arguments: ("Field", "Field")')


def test_value_numbering_and_arguments(hosts):
    h = hosts["ppp"]
    T = h.f["T"]

    def twice(i, j, k, grid, c, p, loc):
        assert p == {"a": 2.0} and loc is Ce                       # everything that is no Field arrives untouched
        return (c[i + 1, j, k] + c[i + 1, j, k]) * p["a"] + (c[i + 1, j, k] + c[i + 1, j, k]) * p["a"]
    prog = ocn.KernelFunctionOperation(CCC, twice, h.grid, T, {"a": 2.0}, Ce).stencil.program
    assert [ins[0] for ins in prog] == [OP["load"], OP["+"], OP["const"], OP["*"], OP["+"]]
    assert sum(ins[0] == OP["load"] for ins in prog) == 1
    # the same Field twice is one argument slot; a function that returns a number is one instruction
    both = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, a, b: a[i, j, k] * b[i, j, k], h.grid, T, T).stencil
    assert len(both.fields) == 1 and [ins[0] for ins in both.program] == [OP["load"], OP["*"]]
    const = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid: 7, h.grid).stencil
    assert const.program == [(OP["const"], 0, 0, 0, 0, 0, 0, 7.0)] and const.fields == []
    # the result is the LAST value even when it was recorded earlier
    early = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: (c[i, j, k], c[i, j, k] * 2.0)[0], h.grid, T).stencil.program
    assert early[-1][:3] == (OP["max"], 0, 0)
    # nothing is simplified: x * 1 and x + 0 stay
    kept = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j, k] * 1 + 0, h.grid, T).stencil.program
    assert [ins[0] for ins in kept] == [OP["load"], OP["const"], OP["*"], OP["const"], OP["+"]]


def test_misused_symbols_are_type_errors(hosts):
    h = hosts["ppp"]
    T = h.f["T"]
    for fn in (lambda i, j, k, grid, c: c[i, j, k] * i, lambda i, j, k, grid, c: c[i * 2, j, k], lambda i, j, k, grid, c: c[i, j, k] + float(k),
               lambda i, j, k, grid, c: i, lambda i, j, k, grid, c: c[i + 0.5, j, k], lambda i, j, k, grid, c: c[i, j, k] if i > 0 else 0.0):
        with pytest.raises(TypeError, match="index symbol"):
            ocn.KernelFunctionOperation(CCC, fn, h.grid, T)
    for fn in (lambda i, j, k, grid, c: c * 2, lambda i, j, k, grid, c: c + c[i, j, k], lambda i, j, k, grid, c: c, lambda i, j, k, grid, c: abs(c)):
        with pytest.raises(TypeError, match="without indexing"):
            ocn.KernelFunctionOperation(CCC, fn, h.grid, T)
    for fn in (lambda i, j, k, grid, c: c[j, i, k], lambda i, j, k, grid, c: c[i, j], lambda i, j, k, grid, c: c[1, 1, 1]):
        with pytest.raises(TypeError, match="indexed with the three index symbols"):
            ocn.KernelFunctionOperation(CCC, fn, h.grid, T)
    with pytest.raises(TypeError, match="truth value"):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: 1.0 if c[i, j, k] > 0 else 0.0, h.grid, T)
    with pytest.raises(TypeError):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: "x", h.grid, T)
    with pytest.raises(TypeError, match="callable"):
        ocn.KernelFunctionOperation(CCC, 3.0, h.grid, T)
    with pytest.raises(ValueError, match="Center / Face"):
        ocn.KernelFunctionOperation((Ce, Ce), lambda *a: 1.0, h.grid)


# ---------------------------------------------------------------------------------------------------------------------
# slots
# ---------------------------------------------------------------------------------------------------------------------
def random_program(rng, n, nargs):
    prog = []
    for q in range(n):
        kinds = ["load", "const"] if q < 2 else ["load", "const", "+", "*", "-", "neg", "select", "max", "sqrt"]
        kind = kinds[rng.integers(len(kinds))]
        if kind == "load":
            prog.append((OP["load"], int(rng.integers(nargs)), 0, 0, int(rng.integers(-1, 2)), 0, 0, 0.0))
        elif kind == "const":
            prog.append((OP["const"], 0, 0, 0, 0, 0, 0, float(q)))
        else:
            ops = [int(rng.integers(q)) for _ in range(O.ARITY[kind])] + [0, 0]
            prog.append((OP[kind], ops[0], ops[1], ops[2], 0, 0, 0, 0.0))
    return prog


def test_slot_plan_equals_the_restated_linear_scan(hosts):
    programs = []
    for name in ("bpb_stretched", "ppp"):
        for diag in R.KERNEL_FUNCTIONS:
            programs.append(named(hosts[name], diag)[0].stencil.program)
    rng = np.random.default_rng(5)
    programs += [random_program(rng, int(rng.integers(3, 120)), 3) for _ in range(20)]
    most = 0
    for prog in programs:
        slots, nslots = O.plan(prog, 3)
        assert (slots, nslots) == R.plan_slots(prog)
        R.assert_no_shared_live_slot(prog, slots)
        assert nslots <= len(prog)
        most = max(most, nslots)
    assert most > 8                                                # the random programs do keep values alive
    strain = named(hosts["bpb_stretched"], "strain")[0].stencil
    print(f"ΣᵢⱼΣᵢⱼᶜᶜᶜ on a stretched grid: {len(strain.program)} instructions, {strain.nslots} live slots")
    assert len(strain.program) <= O.MAX_INSTRUCTIONS and strain.nslots <= 32


def test_limits(hosts):
    h = hosts["ppp"]
    T = h.f["T"]

    def long_chain(i, j, k, grid, c):
        x = c[i, j, k]
        for q in range(O.MAX_INSTRUCTIONS):
            x = x + float(q)
        return x
    with pytest.raises(ValueError, match="256 instructions"):
        ocn.KernelFunctionOperation(CCC, long_chain, h.grid, T)
    # 65 values alive at once: 65 distinct products, all summed afterwards (the instruction count stays under the limit)
    def wide(i, j, k, grid, c):
        xs = [c[i, j, k] * float(q + 2) for q in range(O.MAX_SLOTS + 1)]
        s = xs[0]
        for x in xs[1:]:
            s = s + x
        return s
    with pytest.raises(ValueError, match="64 live values"):
        ocn.KernelFunctionOperation(CCC, wide, h.grid, T)
    nine = [ocn.Field(CCC, h.grid, data=C.c_void_p(0)) for _ in range(9)]
    with pytest.raises(ValueError, match="8 arguments"):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, *c: c[0][i, j, k], h.grid, *nine)
    # the library's own answers, through the planner (no device)
    bad = [(OP["load"], 3, 0, 0, 0, 0, 0, 0.0)]
    for prog, nargs, word in ((bad, 3, "argument slot"), ([(1, 0, 0, 0, 0, 0, 0, 0.0)], 0, "unknown op"), ([(24, 0, 0, 0, 0, 0, 0, 0.0)], 0, "unknown op"),
                              ([(OP["+"], 0, 0, 0, 0, 0, 0, 0.0)], 0, "earlier value"), ([(OP["const"], 0, 0, 0, 1, 0, 0, 0.0)], 0, "offset"),
                              ([(OP["const"], 0, 2, 0, 0, 0, 0, 0.0)], 0, "unused operand"), ([(OP["node"], 3, 0, 0, 0, 0, 0, 0.0)], 0, "direction"),
                              ([(OP["spacing"], 2, 0, 0, 1, 0, 0, 0.0)], 0, "offset"), ([], 0, "1..256")):
        with pytest.raises(ValueError, match=word):
            O.plan(prog, nargs)


# ---------------------------------------------------------------------------------------------------------------------
# the reach rule, Flat directions
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_rule(hosts):
    h = hosts["bpb_stretched"]                                     # halos (3, 3, 3), x and z Bounded
    T, u = h.f["T"], h.f["u"]
    g = h.grid
    ok = lambda loc, fn, *a: ocn.KernelFunctionOperation(loc, fn, g, *a)                  # noqa: E731
    ok(CCC, lambda i, j, k, grid, c: c[i + 3, j - 3, k + 3] + c[i - 3, j + 3, k - 3], T)
    for fn, word in ((lambda i, j, k, grid, c: c[i + 4, j, k], "along x .* needs a halo of 4; the grid has 3"),
                     (lambda i, j, k, grid, c: c[i, j - 4, k], "along y .* needs a halo of 4"),
                     (lambda i, j, k, grid, c: c[i, j, k - 5], "along z .* needs a halo of 5")):
        with pytest.raises(ValueError, match=word):
            ok(CCC, fn, T)
    # a Center argument read from a Face output on a Bounded direction has one point less of room: 71 output points, 70 of the argument
    ok(FCC, lambda i, j, k, grid, c: c[i + 2, j, k] + c[i - 3, j, k], T)
    with pytest.raises(ValueError, match=r"argument 0 read at offset \+3 along x \(71 output points, 70 of the argument\) needs a halo of 4"):
        ok(FCC, lambda i, j, k, grid, c: c[i + 3, j, k], T)
    # ... and the other way round there is one more: a Face argument from a Center output
    ok(CCC, lambda i, j, k, grid, c: c[i + 4, j, k], u)
    with pytest.raises(ValueError, match="halo of 4"):
        ok(CCC, lambda i, j, k, grid, c: c[i - 4, j, k], u)
    # on the Periodic direction Face and Center have the same extent
    ok(CFC, lambda i, j, k, grid, c: c[i, j + 3, k], T)
    with pytest.raises(ValueError, match="along y"):
        ok(CFC, lambda i, j, k, grid, c: c[i, j + 4, k], T)
    # Δz of the stretched grid and the nodes are tables with their own lengths
    ok(CCF, lambda i, j, k, grid: O.Δzᶜᶜᶠ(i, j, k + 3, grid) + O.Δzᶜᶜᶜ(i, j, k - 3, grid))
    with pytest.raises(ValueError, match="Δz read at offset"):
        ok(CCC, lambda i, j, k, grid: O.Δzᶜᶜᶜ(i, j, k + 5, grid))
    ok(CCC, lambda i, j, k, grid: O.xnode(i + 1, j, k, grid, Fa, Ce, Ce) + O.znode(i, j, k, grid, Ce, Ce, Ce))
    for fn in (lambda i, j, k, grid: O.xnode(i - 1, j, k, grid, Ce, Ce, Ce), lambda i, j, k, grid: O.znode(i, j, k + 1, grid, Ce, Ce, Ce)):
        with pytest.raises(ValueError, match="node at offset"):
            ok(CCC, fn)
    with pytest.raises(ValueError, match="node at offset"):       # 71 face outputs, 70 centre nodes
        ok(FCC, lambda i, j, k, grid: O.xnode(i, j, k, grid, Ce, Ce, Ce))
    # the halo of the grid decides, not a literal 3
    h5 = hosts["halo_534"]
    ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i - 5, j + 3, k + 4], h5.grid, h5.f["T"])
    with pytest.raises(ValueError, match="along y .* needs a halo of 4; the grid has 3"):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j + 4, k], h5.grid, h5.f["T"])


def test_flat_direction_rules(hosts):
    h = hosts["slice"]
    g, T, v = h.grid, h.f["T"], h.f["v"]
    I = (O.Index(0), O.Index(1), O.Index(2))
    assert O.δyᵃᶜᵃ(*I, g, T) == 0.0 and O.δyᶜᶠᶜ(*I, g, lambda *a: 1 / 0) == 0.0 and O.dyᶜᶠᶜ(*I, g, T) == 0.0
    assert O.Δyᶜᶜᶜ(*I, g) == 1.0 and O.Δy_invᶜᶠᶜ(*I, g) == 1.0 and O.Azᶜᶜᶜ(*I, g) == g.Δxᶜᵃᵃ and O.Vᶜᶜᶜ(*I, g) == g.Δxᶜᵃᵃ * (1 / 16)
    ident = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: O.ℑyᵃᶜᵃ(i, j, k, grid, c) + O.ℑxyᶜᶜᵃ(i, j, k, grid, c), g, v).stencil.program
    assert [ins[0] for ins in ident] == [OP["load"], OP["load"], OP["+"], OP["const"], OP["*"], OP["+"]]      # ℑy is the identity
    with pytest.raises(ValueError, match="along y, which is Flat"):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j + 1, k], g, T)
    assert O.ℑxᶜᵃᵃ(*I, g, 3.5) == 3.5 and O.dxᶜᶜᶜ(*I, g, 2.0) == 0.0                                     # numbers


# ---------------------------------------------------------------------------------------------------------------------
# interpreter == slices
# ---------------------------------------------------------------------------------------------------------------------
# strain_squared of tests/smagorinsky_reference.py shifts along y: it has no Flat y, so that pair is no case
@pytest.mark.parametrize("grid_name, name", [(g, n) for g in GRIDS for n in R.KERNEL_FUNCTIONS if (g, n) != ("slice", "strain")])
def test_interpreter_equals_slices(hosts, grid_name, name):
    h = hosts[grid_name]
    k, parents = named(h, name)
    got = R.interpret(k.stencil.program, h.grid, k.location, parents)
    want = R.SLICES[name](h.grid, *parents)
    assert got.shape == want.shape == h.grid.interior_size(k.location) and np.array_equal(got, want)
    assert np.isfinite(want).all() and (name == "znode" or np.unique(want).size > want.size // 2)


# ---------------------------------------------------------------------------------------------------------------------
# tree nodes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name", list(GRIDS))
def test_lowering_of_tree_nodes_against_slices(hosts, grid_name):
    h = hosts[grid_name]
    g, T, u, v, w = h.grid, h.f["T"], h.f["u"], h.f["v"], h.f["w"]
    p = h.p

    def value(node):
        st = diagnostics.lower(node)
        return R.interpret(st.program, g, st.location, h.parents(st))
    d = ocn.dz(T)
    assert isinstance(d, ocn.Derivative) and d.location == CCF and d.operator == "dzᶜᶜᶠ" and d.interp == "identity"
    assert np.array_equal(value(d), R.dzT(g, p["T"]))
    m = w * ocn.dz(T)
    assert isinstance(m, ocn.BinaryOperation) and m.location == CCF and not m.fixed and (w * u).fixed
    assert np.array_equal(value(m), R.w_dzT_ccf(g, p["w"], p["T"]))
    c = ocn.at(CCC, w * ocn.dz(T))
    assert c.location == CCC and c.interp_a == "ℑzᵃᵃᶜ" and c.b.location == CCC and c.b.interp == "ℑzᵃᵃᶜ" and c.b.derivative_location == CCF
    assert np.array_equal(value(c), R.w_dzT_ccc(g, p["w"], p["T"]))
    ζ = ocn.dx(v) - ocn.dy(u)
    assert ζ.location == FFC and ζ.interp_a == ζ.interp_b == "identity"
    S = R.Slices(g, FFC)
    want = S.δ(0, lambda s: S(p["v"], s, 0, 0), 0, -1) * (1 / S.dx) - S.δ(1, lambda s: S(p["u"], 0, s, 0), 0, -1) * (1 / S.dy)
    assert np.array_equal(value(ζ), want)
    S = R.Slices(g, FCC)
    assert np.array_equal(value(ocn.sqrt(u * u)), np.sqrt(S(p["u"]) * S(p["u"])))
    assert np.array_equal(value(-T), -R.Slices(g, CCC)(p["T"])) and np.array_equal(value(abs(T)), np.abs(R.Slices(g, CCC)(p["T"])))
    # a Field moved by at(): interpolate_identity; at its own location it stays the Field
    moved = ocn.at(CCC, u)
    assert isinstance(moved, ocn.UnaryOperation) and moved.op == "identity" and moved.interp == "ℑxᶜᵃᵃ" and ocn.at(FCC, u) is u
    S = R.Slices(g, CCC)
    assert np.array_equal(value(moved), 0.5 * (S(p["u"]) + S(p["u"], 1, 0, 0)))
    # a unary operation is op FIRST, interpolation after (unary_operations.jl:21): ℑx(exp(u)), not exp(ℑx(u))
    e = ocn.UnaryOperation("exp", u, CCC)
    assert np.array_equal(value(e), 0.5 * (np.exp(S(p["u"])) + np.exp(S(p["u"], 1, 0, 0))))
    # a derivative of an operation evaluates the inner node at the shifted points
    dd = ocn.dx(u * T)
    assert dd.location == CCC
    uT = lambda s: S(p["u"], s, 0, 0) * (0.5 * (S(p["T"], s - 1, 0, 0) + S(p["T"], s, 0, 0)))       # noqa: E731
    assert np.array_equal(value(dd), (uT(1) - uT(0)) * (1 / S.dx))
    # the three-direction interpolation nests x of y of z, as diagnostics.interpolation_operator names it
    FFF = (Fa, Fa, Fa)
    if grid_name != "slice":
        t = ocn.UnaryOperation("identity", T, FFF)
        assert t.interp == "ℑxyzᶠᶠᶠ"
        S = R.Slices(g, FFF)
        z = lambda di, dj: 0.5 * (S(p["T"], di, dj, -1) + S(p["T"], di, dj, 0))             # noqa: E731
        y = lambda di: 0.5 * (z(di, -1) + z(di, 0))                                          # noqa: E731
        assert np.array_equal(value(t), 0.5 * (y(-1) + y(0)))


def test_locations_names_and_defaults(hosts):
    h = hosts["ppp"]
    T, u, w = h.f["T"], h.f["u"], h.f["w"]
    assert ocn.dx(T).location == FCC and ocn.dx(u).location == CCC and ocn.dy(T).location == CFC and ocn.dz(w).location == CCC
    assert ocn.dx(u).operator == "dxᶜᶜᶜ" and ocn.dy(u).operator == "dyᶠᶠᶜ" and ocn.dz(u).operator == "dzᶠᶜᶠ"
    located = ocn.dz(CCC, T)
    assert located.location == CCC and located.derivative_location == CCF and located.interp == "ℑzᵃᵃᶜ"
    assert ocn.sqrt(T).location == CCC and ocn.tanh(ocn.dz(T)).location == CCF and isinstance(ocn.cos(u), ocn.UnaryOperation)
    assert ocn.sqrt(4.0) == 2.0                                     # numbers still go to numpy
    for name in ("δxᶠᵃᵃ", "ℑxyᶠᶜᵃ", "Δzᶜᶜᶠ", "Azᶜᶜᶠ", "Vᶜᶜᶜ", "div_xyᶜᶜᶜ", "dxᶜᶜᶜ", "Δx_invᶜᶜᶜ", "ζ3ᶠᶠᶜ", "δzᶜᶜᶠ", "ℑxyzᶜᶠᶜ", "Ax_qᶠᶜᶜ"):
        assert name.isidentifier() and callable(getattr(O, name)), name
    assert O.dxᶜᶜᶜ.__doc__.startswith("∂xᶜᶜᶜ (Operators/derivative_operators.jl") and O.ζ3ᶠᶠᶜ.__doc__.startswith("ζ₃ᶠᶠᶜ")
    assert O.Δx_invᶠᶜᶜ.__doc__.startswith("Δx⁻¹ᶠᶜᶜ") and O.δxᶠᵃᵃ.__name__ == "δxᶠᵃᵃ"
    for name in ("KernelFunctionOperation", "Derivative", "UnaryOperation", "at", "dx", "dy", "dz", "operators"):
        assert name in ocn.__all__
    # accepted wherever a BinaryOperation is
    k = ocn.KernelFunctionOperation(FFC, O.ζ3ᶠᶠᶜ, h.grid, u, h.f["v"])
    for operand in (k, ocn.dz(T), ocn.sqrt(T), w * ocn.dz(T)):
        loc = operand.location
        assert ocn.Average(operand, dims=(1, 2)).location == (None, None, loc[2]) and ocn.Integral(operand).location == (None,) * 3
        assert ocn.Reduction("maximum", operand, 1).location == (None, loc[1], loc[2])
        assert ocn.CumulativeIntegral(operand, 3).location == loc and ocn.Accumulation("cumsum", operand, 1).location == loc
        lazy = ocn.Field(T.loc, h.grid, data=C.c_void_p(0))
        assert diagnostics.as_field_operand(operand) is operand and lazy.operand is None


def test_refusals(hosts):
    h = hosts["ppp"]
    T, u = h.f["T"], h.f["u"]
    # the pinned refusals of a BinaryOperation's own arithmetic still raise, in their words, and now name the other route
    for make in (lambda: (u * T) * T, lambda: T + (u * T), lambda: 2 * (u * T), lambda: (u * T) ** 2, lambda: ocn.dz(T) * (u * T)):
        with pytest.raises(NotImplementedError, match=r"Field\(op\).*KernelFunctionOperation"):
            make()
    for exponent in (3, 0.5):
        with pytest.raises(NotImplementedError, match="exponent"):
            ocn.dz(T) ** exponent
    for operand in (np.sin, "∂x(u)", np.ones(3)):
        with pytest.raises(NotImplementedError):
            T * operand
        with pytest.raises(NotImplementedError):
            ocn.dz(T) * operand
        with pytest.raises(NotImplementedError):
            ocn.dx(operand)
    for name in ("log10", "tan", "sinh", "cosh"):
        with pytest.raises(NotImplementedError, match=name):
            ocn.UnaryOperation(name, T)
    for kw in ({"condition": lambda *a: True}, {"mask": 0}):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            ocn.Average(ocn.dz(T), **kw)
    reduced = ocn.Field((None, None, Ce), h.grid, data=C.c_void_p(0))
    for make in (lambda: ocn.dz(reduced), lambda: ocn.sqrt(reduced), lambda: ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j, k], h.grid, reduced)):
        with pytest.raises(NotImplementedError, match="reduced field"):
            make()
    k = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j, k], h.grid, T)
    for make in (lambda: k * 2, lambda: T + k, lambda: ocn.dz(k), lambda: ocn.Average(ocn.Average(k, dims=1))):
        with pytest.raises(NotImplementedError):
            make()
    other = GRIDS["ppp"]()
    with pytest.raises(ValueError, match="different grids"):
        ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, c: c[i, j, k], h.grid, other.f["T"])
    with pytest.raises(ValueError, match="different grids"):
        ocn.dz(T) * other.f["T"]
    part = ocn.RectilinearGrid(None, size=(6, 5, 4), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    c = ocn.Field(CCC, part, data=C.c_void_p(0))
    for make in (lambda: ocn.dz(c), lambda: ocn.sqrt(c), lambda: -c, lambda: ocn.KernelFunctionOperation(CCC, lambda *a: 1.0, part)):
        with pytest.raises(NotImplementedError, match="partitioned"):
            make()
