"""Stencil programs on the device (csrc/ocn_diagnostics.h: the DgStencil overload of dg_eval; include/ocn_mi355x.h: ocn_compute_stencil,
ocn_reduce_stencil, ocn_accumulate_stencil) against tests/stencil_reference.py.

Computed fields are compared with `==` on the whole parent, halos included: every instruction is one IEEE operation and the translation
unit is compiled with contraction off, so route (b) of the reference -- numpy slices -- gives the same bits. Extrema and accumulations
have a defined order and are `==` too. A sum of n terms xᵢ passes within n 2⁻⁵³ Σ|xᵢ| of math.fsum of the restatement's terms, an average
within (2n + 2) 2⁻⁵³ Σ|xᵢ| / V (tests/test_gpu_diagnostics.py). Transcendentals are compared in ulps of the numpy value with the bounds
of the boundary functions: exp 3, log 3, sin 4, cos 4, tanh 5, pow 16, plus 1 for numpy's own error."""
import ctypes as C
import math

import numpy as np
import pytest

import diagnostics_reference as D
import halo_cases as HC
import stencil_reference as R
from helpers import tanh_faces
from test_gpu_diagnostics import ALL_DIMS, D_reduced, assert_sum_within_bound

pytestmark = pytest.mark.gpu

CCC, FCC, CFC, CCF, FFC = R.CCC, R.FCC, R.CFC, R.CCF, R.FFC
NAMED = ("dzT", "w_dzT_ccf", "w_dzT_ccc", "vorticity", "kinetic_energy", "divergence", "znode", "strain")


class Case:
    """a grid, the oracle's twin of it (for the halo fill), four random fields and their host parents"""

    def __init__(self, ocn, O, arch, name):
        self.name, halo = name, None
        if name == "bpb_stretched":
            topo, size, kw = ("Bounded", "Periodic", "Bounded"), (70, 37, 9), dict(x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(9))
        elif name == "slice":
            topo, size, kw = ("Bounded", "Flat", "Bounded"), (66, 1, 16), dict(x=(0.0, 1.0), z=(-1.0, 0.0))
        elif name == "ppp":
            topo, size, kw = ("Periodic",) * 3, (16, 16, 16), dict(x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
        else:                                                  # the stretched (Periodic, Periodic, Bounded) grid of halo_cases.py at halos (5, 3, 4)
            topo, size, _ = HC.GRIDS["ppb"]
            kw, halo = dict(x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(size[2])), HC.HALOS[0]
        gkw = dict(kw) if halo is None else dict(kw, halo=halo)
        self.grid = ocn.RectilinearGrid(arch, size=tuple(n for n, t in zip(size, topo) if t != "Flat"), topology=tuple(getattr(ocn, t) for t in topo), **gkw)
        code = {"Periodic": 0, "Bounded": 1, "Flat": 3}
        self.oracle_grid = O.Grid(size, halo=halo, topology=tuple(code[t] for t in topo), x=kw["x"], y=kw.get("y", (0.0, 1.0)), z=kw["z"])
        rng = np.random.default_rng(20250311)
        self.f, self.p = {}, {}
        for n, loc in (("T", CCC), ("u", FCC), ("v", CFC), ("w", CCF)):
            f = ocn.Field(loc, self.grid)
            a = np.asfortranarray(0.5 + rng.standard_normal(f.shape))
            f.set_parent(a)                                    # the halos hold values too
            self.f[n], self.p[n] = f, a
        self.ocn = ocn

    def named(self, name):
        """(KernelFunctionOperation, the interior by route (b))"""
        loc, fn, args = R.KERNEL_FUNCTIONS[name]
        return self.ocn.KernelFunctionOperation(loc, fn, self.grid, *[self.f[a] for a in args]), R.SLICES[name](self.grid, *[self.p[a] for a in args])

    def names(self):
        return [n for n in NAMED if not (n == "strain" and self.name == "slice")]      # strain_squared has no Flat y


GRIDS = ("bpb_stretched", "slice", "ppp", "halo_534")


@pytest.fixture(scope="module")
def cases(ocn, oracle, arch):
    return {n: Case(ocn, oracle, arch, n) for n in GRIDS}


def whole_parent(c, field, interior):
    want = np.zeros(field.shape, order="F")
    want[field._interior_slices()] = interior
    c.oracle_grid.fill_halo_regions(want, [0 if l is c.ocn.Center else 1 for l in field.loc])
    return want


# ---------------------------------------------------------------------------------------------------------------------
# computed fields
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_computed_fields_of_named_diagnostics_equal_the_slices_halos_included(ocn, cases, name):
    c = cases[name]
    for diag in c.names():
        k, interior = c.named(diag)
        f = ocn.Field(k)
        assert f.operand is k and f.loc == k.location and f.shape == c.grid.total_size(k.location)
        got, want = f.parent(), whole_parent(c, f, interior)
        assert np.array_equal(got, want), (name, diag, np.argwhere(got != want)[:4])
        lazy = ocn.Field(k, compute=False)
        assert not lazy.parent().any() and np.array_equal(ocn.compute(lazy).parent(), want)
        ocn.compute_at(lazy, 0.0)                               # the status holds 0: no compute, nothing changes
        assert np.array_equal(lazy.parent(), want)


@pytest.mark.parametrize("name", GRIDS)
def test_tree_nodes_equal_the_slices(ocn, cases, name):
    c = cases[name]
    T, u, v, w = (c.f[n] for n in "Tuvw")
    p = c.p
    S = R.Slices(c.grid, FFC)
    ζ = S.δ(0, lambda s: S(p["v"], s, 0, 0), 0, -1) * (1 / S.dx) - S.δ(1, lambda s: S(p["u"], 0, s, 0), 0, -1) * (1 / S.dy)
    S = R.Slices(c.grid, FCC)
    for node, interior in ((ocn.dz(T), R.dzT(c.grid, p["T"])), (w * ocn.dz(T), R.w_dzT_ccf(c.grid, p["w"], p["T"])),
                           (ocn.at(CCC, w * ocn.dz(T)), R.w_dzT_ccc(c.grid, p["w"], p["T"])), (ocn.dx(v) - ocn.dy(u), ζ),
                           (ocn.sqrt(u * u), np.sqrt(S(p["u"]) * S(p["u"]))), (-u, -S(p["u"])), (abs(u), np.abs(S(p["u"])))):
        f = ocn.Field(node)
        got, want = f.parent(), whole_parent(c, f, interior)
        assert f.loc == node.location and np.array_equal(got, want), (name, node, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", GRIDS)
def test_one_node_through_the_interpreter_equals_the_fixed_evaluator_bitwise(ocn, cases, name):
    c = cases[name]
    T, u, w = c.f["T"], c.f["u"], c.f["w"]
    for op in (w * u, u * w, T - 0.5, 2 / T, u ** 2, T):
        loc = op.location if hasattr(op, "location") else op.loc
        fixed, interpreted = ocn.Field(loc, c.grid), ocn.Field(loc, c.grid)
        ocn.kernels.compute_operation(c.grid, op, fixed)
        ocn.kernels.compute_stencil(c.grid, op, interpreted)
        a = fixed.parent()
        assert a.any() and np.array_equal(a, interpreted.parent()), (name, op)
        for dims in ((1, 2), 3, None):
            dd = (1, 2, 3) if dims is None else ((dims,) if isinstance(dims, int) else dims)
            a, b = ocn.Field(D_reduced(loc, dims), c.grid), ocn.Field(D_reduced(loc, dims), c.grid)
            ocn.kernels.reduce_operation(c.grid, op, "average", dd, 3 in dd and not c.grid.z_regular, False, a)
            ocn.kernels.reduce_stencil(c.grid, op, "average", dd, 3 in dd and not c.grid.z_regular, False, b)
            assert np.array_equal(a.interior(), b.interior()), (name, op, dims)


def ulps(got, want):
    return np.max(np.abs(got - want) / np.spacing(np.abs(want)))


def test_transcendentals_within_their_ulp_bounds(ocn, cases):
    c = cases["bpb_stretched"]
    T = c.f["T"]
    x = R.Slices(c.grid, CCC)(c.p["T"])
    worst = {}
    for name, bound, node, want in (("exp", 3, ocn.exp(T), np.exp(x)), ("log", 3, ocn.log(abs(T)), np.log(np.abs(x))), ("sin", 4, ocn.sin(T), np.sin(x)),
                                    ("cos", 4, ocn.cos(T), np.cos(x)), ("tanh", 5, ocn.tanh(T), np.tanh(x)),
                                    ("pow", 16, ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, a: abs(a[i, j, k]) ** 2.5, c.grid, T), np.abs(x) ** 2.5)):
        got = ocn.Field(node).interior()
        worst[name] = ulps(got, want)
        print(f"{name}: largest error {worst[name]:.2f} ulp (bound {bound} + 1)")
        assert worst[name] <= bound + 1, name
    # a program with transcendentals in a reduction: the other instantiation of the reducing kernels
    terms = np.exp(x) * np.sin(x)
    k = ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, a: ocn.exp(a[i, j, k]) * ocn.sin(a[i, j, k]), c.grid, T)
    got = ocn.Field(ocn.Reduction("maximum", k, (1, 2))).interior()
    want = np.max(terms, axis=(0, 1), keepdims=True)
    assert got.shape == want.shape and ulps(got, want) <= 3 + 4 + 1 + 1          # exp, sin, the product, numpy


# ---------------------------------------------------------------------------------------------------------------------
# reductions and accumulations
# ---------------------------------------------------------------------------------------------------------------------
def _dims(dims):
    return (1, 2, 3) if dims is None else ((dims,) if isinstance(dims, int) else dims)


@pytest.mark.parametrize("name", GRIDS)
def test_extrema_and_accumulations_equal_the_restatement(ocn, cases, name):
    c = cases[name]
    for diag in ("vorticity", "w_dzT_ccc"):
        k, v = c.named(diag)
        for dims in ALL_DIMS:
            ax = tuple(d - 1 for d in _dims(dims))
            for kind, red in (("maximum", np.max), ("minimum", np.min)):
                for f in (None, abs):
                    want = red(np.abs(v) if f is abs else v, axis=ax, keepdims=True)
                    got = ocn.Field(ocn.Reduction(kind, k, dims, f=f))
                    assert got.loc == D_reduced(k.location, dims) and np.array_equal(got.interior(), want), (name, diag, dims, kind, f)
        for dim in (1, 2, 3):
            for reverse in (False, True):
                for scan, metric in ((ocn.CumulativeIntegral(k, dims=dim, reverse=reverse), True), (ocn.Accumulation("cumsum", k, dim, reverse=reverse), False)):
                    a = v * D.metric(c.grid, k.location, 1 << (dim - 1)) if metric else v
                    want = np.flip(np.cumsum(np.flip(a, axis=dim - 1), axis=dim - 1), axis=dim - 1) if reverse else np.cumsum(a, axis=dim - 1)
                    f = ocn.Field(scan)
                    got = f.parent()
                    assert f.loc == k.location and np.array_equal(got[f._interior_slices()], want), (name, diag, dim, reverse, metric)
                    got[f._interior_slices()] = 0
                    assert not got.any()                         # the halos stay as allocated


@pytest.mark.parametrize("name", GRIDS)
def test_sums_integrals_and_averages_within_the_summation_bound(ocn, cases, name):
    c = cases[name]
    worst = 0.0
    for diag in ("vorticity", "w_dzT_ccf", "kinetic_energy"):
        k, v = c.named(diag)
        for dims in ALL_DIMS:
            dd = _dims(dims)
            mask, axes = ocn.diagnostics.dims_mask(dd), tuple(d - 1 for d in dd)
            m = np.broadcast_to(D.metric(c.grid, k.location, mask), v.shape)
            count = int(np.prod([v.shape[d] for d in axes]))
            avg = ocn.Average(k, dims)
            assert avg.use_metric is (3 in dd and not c.grid.z_regular)
            for what, got, terms, average, with_metric in (("Average", ocn.Field(avg).interior(), v * m if avg.use_metric else v, True, avg.use_metric),
                                                           ("Integral", ocn.Field(ocn.Integral(k, dims)).interior(), v * m, False, True),
                                                           ("Reduction sum", ocn.Field(ocn.Reduction("sum", k, dims)).interior(), v, False, False)):
                assert got.shape == tuple(1 if d in axes else v.shape[d] for d in range(3)), (name, diag, dims, what)
                worst = max(worst, assert_sum_within_bound(got, terms, m if with_metric else None, count, axes, average, (name, diag, dims, what)))
    print(f"{name}: largest error / bound = {worst:.3f}")


def test_repeated_computes_give_identical_bits(ocn, cases):
    c = cases["bpb_stretched"]
    for diag in ("strain", "vorticity"):
        k, _ = c.named(diag)
        for dims in ((1, 2), None, 1, (1, 3)):
            f = ocn.Field(ocn.Average(k, dims))
            first = f.parent()
            for _ in range(3):
                assert np.array_equal(ocn.compute(f).parent(), first), (diag, dims)
            assert np.array_equal(ocn.Field(ocn.Average(k, dims)).parent(), first)


def test_a_program_with_more_than_32_live_values(ocn, cases):
    """48 products alive at once (49 slots, 98 KiB of LDS): more than a launch gets without asking"""
    c = cases["ppp"]
    T = c.f["T"]

    def wide(i, j, k, grid, a):
        xs = [a[i, j, k] * float(q + 2) for q in range(48)]
        s = xs[0]
        for x in xs[1:]:
            s = s + x
        return s
    k = ocn.KernelFunctionOperation(CCC, wide, c.grid, T)
    assert 32 < k.stencil.nslots <= 64
    x = R.Slices(c.grid, CCC)(c.p["T"])
    want = x * 2.0
    for q in range(1, 48):
        want = want + x * float(q + 2)
    assert np.array_equal(ocn.Field(k).interior(), want)
    assert np.array_equal(ocn.Field(ocn.Reduction("maximum", k, (1, 2))).interior(), np.max(want, axis=(0, 1), keepdims=True))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's data-free checks (test/test_computed_field.jl)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(ocn, arch):
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    return ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))


def isapprox(a, b):
    """Julia's ≈ of two numbers: rtol = √eps"""
    return np.abs(a - b) <= math.sqrt(np.finfo(np.float64).eps) * np.maximum(np.abs(a), np.abs(b))


def test_reference_compute_derivative_and_unary(ocn, model):
    """compute_derivative (test_computed_field.jl:3-9) and compute_unary (:11-17)"""
    S = model.fields()["S"]
    S.set_parent(np.full(S.shape, np.pi))
    for d in (ocn.dx, ocn.dy, ocn.dz):
        assert np.all(ocn.Field(d(S)).interior() == 0)
    ocn.set_model(model, S=np.pi)
    for unary, f in ((ocn.sqrt, math.sqrt), (ocn.sin, math.sin), (ocn.cos, math.cos), (ocn.exp, math.exp), (ocn.tanh, math.tanh), (abs, abs),
                     (lambda x: -x, lambda x: -x)):
        assert np.all(isapprox(ocn.Field(unary(S)).interior(), f(np.pi)))


def test_reference_compute_kinetic_energy(ocn, model):
    """compute_kinetic_energy (:52-62): the kernel function of (u² + v² + w²) / 2 at ccc"""
    f = model.fields()
    for n, value in (("u", 1.0), ("v", 2.0), ("w", 3.0)):
        f[n].set(value)
    ocn.fill_halo_regions([f["u"], f["v"], f["w"]])
    ke = ocn.Field(ocn.KernelFunctionOperation(CCC, R.kinetic_energy_kernel, model.grid, f["u"], f["v"], f["w"]))
    assert np.all(isapprox(ke.interior()[1:3, 1:3, 1:3], 7.0))


def test_reference_multiplication_and_derivative(ocn, model):
    """multiplication_and_derivative_ccf / _ccc (:149-194), with the reference's omitted boundary points"""
    Nz = model.grid.Nz
    ocn.set_model(model, enforce_incompressibility=False, w=lambda x, y, z: np.sin(np.pi * z) + 0 * x + 0 * y, T=lambda x, y, z: 42 * z + 0 * x + 0 * y)
    f = model.fields()
    w, T = f["w"], f["T"]
    zF = model.grid.nodes(CCF)[2].reshape(-1)
    wT = ocn.Field(ocn.Average(w * ocn.dz(T), dims=(1, 2))).interior()[0, 0, :Nz]
    correct = 42 * np.sin(np.pi * zF)
    assert np.all(isapprox(wT[1:Nz], correct[1:Nz]))
    ccc = ocn.Field(ocn.Average(ocn.at(CCC, w * ocn.dz(T)), dims=(1, 2))).interior()
    sinusoid = np.sin(np.pi * zF)
    correct = np.array([(sinusoid[k] + sinusoid[k + 1]) / 2 for k in range(Nz)]) * 42
    assert ccc.shape == (1, 1, Nz) and np.all(isapprox(ccc[0, 0, 1:Nz - 1], correct[1:Nz - 1]))


def test_diagnostics_of_a_model_leave_it_untouched(ocn, arch):
    def make():
        grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        m = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T",))
        rng = np.random.default_rng(7)
        ocn.set_model(m, **{n: 0.1 * rng.standard_normal(m.grid.interior_size(f.loc)) for n, f in m.fields().items()})
        return m
    m, twin = make(), make()
    dt = 0.1 * m.grid.Δxᶜᵃᵃ / 0.6
    for mm in (m, twin):
        for _ in range(2):
            ocn.time_step(mm, dt)
    f = m.fields()
    before = {n: a.parent() for n, a in f.items()}
    u, v, w, T = f["u"], f["v"], f["w"], f["T"]
    ζ = ocn.Field(ocn.KernelFunctionOperation(FFC, ocn.operators.ζ3ᶠᶠᶜ, m.grid, u, v))
    assert np.array_equal(ζ.interior(), R.vorticity(m.grid, before["u"], before["v"]))
    Σ = ocn.Field(ocn.Average(ocn.KernelFunctionOperation(CCC, R.ΣᵢⱼΣᵢⱼᶜᶜᶜ, m.grid, u, v, w), dims=(1, 2))).interior()
    terms = R.strain(m.grid, before["u"], before["v"], before["w"])
    assert_sum_within_bound(Σ, terms, None, 256, (0, 1), True, "model")
    ocn.Field(ocn.CumulativeIntegral(w * ocn.dz(T), 3))
    for n, a in f.items():
        assert np.array_equal(a.parent(), before[n]), n
    for mm in (m, twin):
        for _ in range(2):
            ocn.time_step(mm, dt)
    for n, a in f.items():
        assert np.array_equal(a.parent(), twin.fields()[n].parent()), n


# ---------------------------------------------------------------------------------------------------------------------
# the raw C ABI: refusals by return code, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_refuse_bad_programs(ocn, arch, cases):
    from oldoceananigans_jl_amd import _lib, operators as O
    L = _lib.lib()
    EINVAL, ENOTSUP, ESTATE = -1, -2, -3
    OP = O.OPS

    def operand(grid, program, fields, loc):
        s = _lib.StencilOperand()
        arr, s.n = O.program_array(program)
        s.program = arr
        ptrs = (C.c_void_p * max(len(fields), 1))(*[f.data for f in fields])
        locs = (C.c_int * (3 * max(len(fields), 1)))(*[x for f in fields for x in f.loc_codes])
        s.args, s.arg_locs, s.nargs = ptrs, locs, len(fields)
        s.loc[:] = [l.code for l in loc]
        return s, (arr, ptrs, locs)

    c = cases["bpb_stretched"]
    T, u = c.f["T"], c.f["u"]
    out = ocn.Field(FCC, c.grid)
    load = lambda slot, di=0, dj=0, dk=0: (OP["load"], slot, 0, 0, di, dj, dk, 0.0)                     # noqa: E731

    def refused(grid, program, fields, loc, code, word, dst=out):
        s, keep = operand(grid, program, fields, loc)
        for call in (lambda: L.ocn_compute_stencil(grid.handle, C.byref(s), dst.data), lambda: L.ocn_reduce_stencil(grid.handle, C.byref(s), 0, 3, 0, 0, dst.data),
                     lambda: L.ocn_accumulate_stencil(grid.handle, C.byref(s), 0, 0, 0, dst.data)):
            assert call() == code and word in L.ocn_last_error(), (program, L.ocn_last_error())

    # the reach rule: |off| <= H is not enough for a Center argument read from a Face output on a Bounded direction
    refused(c.grid, [load(0, 3)], [T], FCC, EINVAL, b"needs a halo of 4")
    refused(c.grid, [load(0, -4)], [T], CCC, EINVAL, b"needs a halo of 4")
    refused(c.grid, [load(0, 0, 0, 4)], [T], CCC, EINVAL, b"along z")
    refused(c.grid, [(OP["spacing"], 2, 0, 0, 0, 0, 5, 0.0)], [], CCC, EINVAL, b"z read at offset")
    refused(c.grid, [(OP["node"], 0, 0, 0, 0, 0, 0, 0.0)], [], FCC, EINVAL, b"node at offset")
    refused(c.grid, [(OP["node"], 2, 1, 0, 0, 0, -1, 0.0)], [], CCC, EINVAL, b"node at offset")
    # program errors
    refused(c.grid, [(1, 0, 0, 0, 0, 0, 0, 0.0)], [], CCC, EINVAL, b"unknown op")
    refused(c.grid, [(24, 0, 0, 0, 0, 0, 0, 0.0)], [], CCC, EINVAL, b"unknown op")
    refused(c.grid, [(99, 0, 0, 0, 0, 0, 0, 0.0)], [], CCC, EINVAL, b"unknown op")
    refused(c.grid, [load(1)], [T], CCC, EINVAL, b"argument slot 1")
    refused(c.grid, [load(0), (OP["+"], 0, 1, 0, 0, 0, 0, 0.0)], [T], CCC, EINVAL, b"earlier value")
    refused(c.grid, [load(0), (OP["neg"], 0, 0, 0, 1, 0, 0, 0.0)], [T], CCC, EINVAL, b"offset")
    refused(c.grid, [], [], CCC, EINVAL, b"1..256")
    s, keep = operand(c.grid, [load(0)], [T], CCC)
    s.loc[0] = 7
    assert L.ocn_compute_stencil(c.grid.handle, C.byref(s), out.data) == EINVAL and b"loc[0]" in L.ocn_last_error()
    s, keep = operand(c.grid, [load(0)], [T], CCC)
    for call in (lambda: L.ocn_compute_stencil(c.grid.handle, None, out.data), lambda: L.ocn_compute_stencil(c.grid.handle, C.byref(s), None),
                 lambda: L.ocn_compute_stencil(None, C.byref(s), out.data), lambda: L.ocn_reduce_stencil(c.grid.handle, C.byref(s), 0, 3, 0, 0, None)):
        assert call() == EINVAL and b"NULL" in L.ocn_last_error()
    assert L.ocn_reduce_stencil(c.grid.handle, C.byref(s), 0, 0, 0, 0, out.data) == EINVAL and b"dims_mask" in L.ocn_last_error()
    assert L.ocn_reduce_stencil(c.grid.handle, C.byref(s), 1, 1, 1, 0, out.data) == EINVAL
    assert L.ocn_accumulate_stencil(c.grid.handle, C.byref(s), 3, 0, 0, out.data) == EINVAL
    # an offset along a Flat direction
    sl = cases["slice"]
    refused(sl.grid, [load(0, 0, 1)], [sl.f["T"]], CCC, EINVAL, b"which is Flat", dst=ocn.Field(CCC, sl.grid))
    ocn.synchronize()
    assert not out.parent().any()                                    # nothing was launched
    # a connected (partitioned) handle is refused by the library itself
    part = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    pc, pout = ocn.Field(CCC, part), ocn.Field(CCC, part)
    refused(part, [load(0)], [pc], CCC, ENOTSUP, b"partitioned", dst=pout)
    # a grid handle that never got its node tables: OCN_ESTATE for a NODE, everything else is served
    bare = C.c_void_p()
    _lib.check(L.ocn_grid_create(C.byref(bare), _lib.i3((16, 16, 16)), _lib.i3((3, 3, 3)), _lib.i3((0, 0, 1)), (C.c_double * 3)(1.0, 1.0, 1.0),
                                 1 / 16, 1 / 16, 1 / 16, None, None))
    try:
        g16 = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        dst = ocn.Field(CCC, g16)
        s, keep = operand(g16, [(OP["node"], 2, 0, 0, 0, 0, 0, 0.0)], [], CCC)
        assert L.ocn_compute_stencil(bare, C.byref(s), dst.data) == ESTATE and b"node tables" in L.ocn_last_error()
        ocn.synchronize()
        assert not dst.parent().any()
    finally:
        L.ocn_grid_destroy(bare)
