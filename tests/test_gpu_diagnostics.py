"""GPU tests of the diagnostics (csrc/ocn_diagnostics.h through oldoceananigans_jl_amd/diagnostics.py) against the numpy restatement
tests/diagnostics_reference.py, which tests/test_diagnostics_host.py pins to the reference's numbers.

Computed fields, accumulations and extrema have a defined operation order: compared with `==`. Sums are compared per output element with
S = math.fsum of the restatement's n terms xᵢ: a sum passes within n 2⁻⁵³ Σ|xᵢ| of S, an average within (2n + 2) 2⁻⁵³ Σ|xᵢ| / V of S / V
(V the count or the fsum of the metric) -- the worst-case bound of a floating-point sum in ANY order, plus the divisor's own sum and the
division. Derived, not measured: a dropped or doubled term exceeds it by many orders at these sizes.

Grids: the smallest that exercise the kernels -- rows longer than a wave and no multiple of 64 (70, 71 for u), more than ten 256-thread
blocks per level, more rows per output than one chunk (37 > 16), a stretched z, a Flat direction."""
import ctypes as C
import math

import numpy as np
import pytest

import diagnostics_reference as D
from helpers import tanh_faces

pytestmark = pytest.mark.gpu

ALL_DIMS = (1, 2, 3, (1, 2), (1, 3), (2, 3), None)
U = 2.0 ** -53


class Case:
    """a grid, the oracle's twin of it (for the halo fill), four random fields and their host parents"""

    def __init__(self, ocn, O, arch, name):
        self.name = name
        Ce, Fa = ocn.Center, ocn.Face
        if name == "bpb_stretched":
            topo, size, kw = ("Bounded", "Periodic", "Bounded"), (70, 37, 9), dict(x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(9))
        elif name == "slice":
            topo, size, kw = ("Bounded", "Flat", "Bounded"), (66, 1, 16), dict(x=(0.0, 1.0), z=(-1.0, 0.0))
        else:
            topo, size, kw = ("Periodic",) * 3, (16, 16, 16), dict(x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
        self.grid = ocn.RectilinearGrid(arch, size=tuple(n for n, t in zip(size, topo) if t != "Flat"), topology=tuple(getattr(ocn, t) for t in topo), **kw)
        code = {"Periodic": 0, "Bounded": 1, "Flat": 3}
        self.oracle_grid = O.Grid(size, topology=tuple(code[t] for t in topo), x=kw["x"], y=kw.get("y", (0.0, 1.0)), z=kw["z"])
        rng = np.random.default_rng(20240607)
        self.parents, self.fields = {}, {}
        for n, loc in (("T", (Ce, Ce, Ce)), ("u", (Fa, Ce, Ce)), ("v", (Ce, Fa, Ce)), ("w", (Ce, Ce, Fa))):
            f = ocn.Field(loc, self.grid)
            a = np.asfortranarray(0.5 + rng.standard_normal(f.shape))
            f.set_parent(a)                                    # the halos hold values too
            self.fields[n], self.parents[f] = f, a

    def operands(self, names):
        T, u, v, w = (self.fields[n] for n in "Tuvw")
        table = {"T": T, "u": u, "w": w, "w*u": w * u, "u*w": u * w, "T*w": T * w, "u+v": u + v, "T-0.5": T - 0.5, "2/T": 2 / T, "u**2": u ** 2}
        return [(n, table[n]) for n in names]

    def location(self, operand):
        return operand.location if hasattr(operand, "interp_a") else operand.loc


@pytest.fixture(scope="module")
def cases(ocn, oracle, arch):
    return {n: Case(ocn, oracle, arch, n) for n in ("bpb_stretched", "slice", "ppp")}


GRIDS = ("bpb_stretched", "slice", "ppp")


# ---------------------------------------------------------------------------------------------------------------------
# computed fields
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_computed_fields_equal_the_restatement_halos_included(ocn, cases, name):
    c = cases[name]
    for label, op in c.operands(("w*u", "u*w", "T*w", "u+v", "T-0.5", "2/T", "u**2")):
        f = ocn.Field(op)
        assert f.operand is op and f.loc == op.location and f.shape == c.grid.total_size(op.location)
        want = np.zeros(f.shape, order="F")
        want[f._interior_slices()] = D.compute_operation(c.grid, D.operand_of(op, c.parents))
        c.oracle_grid.fill_halo_regions(want, [0 if l is ocn.Center else 1 for l in op.location])
        got = f.parent()
        assert np.array_equal(got, want), (name, label, np.argwhere(got != want)[:4])
        lazy = ocn.Field(op, compute=False)
        assert not lazy.parent().any()
        assert np.array_equal(ocn.compute(lazy).parent(), want)


# ---------------------------------------------------------------------------------------------------------------------
# scans with a defined order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_accumulations_in_the_sequential_order(ocn, cases, name):
    c = cases[name]
    for label, op in c.operands(("T", "u", "w", "w*u")):
        operand = D.operand_of(op, c.parents)
        for dim in (1, 2, 3):
            for reverse in (False, True):
                for scan, metric in ((ocn.CumulativeIntegral(op, dims=dim, reverse=reverse), True), (ocn.Accumulation("cumsum", op, dim, reverse=reverse), False)):
                    f = ocn.Field(scan)
                    assert f.loc == tuple(c.location(op))
                    want = D.accumulate_operation(c.grid, operand, dim - 1, reverse, metric)
                    got = f.parent()
                    assert np.array_equal(got[f._interior_slices()], want), (name, label, dim, reverse, metric)
                    got[f._interior_slices()] = 0
                    assert not got.any()                         # the halos stay as allocated


@pytest.mark.parametrize("name", GRIDS)
def test_extrema_on_all_dims(ocn, cases, name):
    c = cases[name]
    for label, op in c.operands(("u", "w*u")):
        operand = D.operand_of(op, c.parents)
        for dims in ALL_DIMS:
            mask = ocn.diagnostics.dims_mask((1, 2, 3) if dims is None else ((dims,) if isinstance(dims, int) else dims))
            for kind in ("maximum", "minimum"):
                for f in (None, abs):
                    want = D.reduce_operation(c.grid, operand, kind, mask, False, f is abs)
                    got = ocn.Field(ocn.Reduction(kind, op, dims, f=f))
                    assert got.loc == D_reduced(c.location(op), dims) and np.array_equal(got.interior(), want), (name, label, dims, kind, f)
                    if not hasattr(op, "interp_a"):
                        alloc = getattr(op, kind)(dims=dims, f=f)
                        assert (alloc == want[0, 0, 0]) if dims is None else np.array_equal(alloc.interior(), want)


def D_reduced(loc, dims):
    dims = (1, 2, 3) if dims is None else ((dims,) if isinstance(dims, int) else dims)
    return tuple(None if d + 1 in dims else l for d, l in enumerate(loc))


# ---------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------
def _rows(a, axes):
    """(outputs, terms) with the reduced axes last"""
    kept = [d for d in range(3) if d not in axes]
    return np.transpose(a, kept + list(axes)).reshape(int(np.prod([a.shape[d] for d in kept])), -1)


def assert_sum_within_bound(got, terms, metric, count, axes, average, tag):
    """got: the reduced interior; the bounds of the module docstring, every figure printed before it is asserted"""
    x = _rows(terms, axes)
    m = _rows(metric, axes) if metric is not None else None
    g = _rows(got, ())[:, 0] if got.ndim == 3 else np.asarray(got).reshape(-1)
    assert g.size == x.shape[0], tag
    n = x.shape[1]
    worst = 0.0
    for q in range(x.shape[0]):
        S, A = math.fsum(x[q].tolist()), math.fsum(np.abs(x[q]).tolist())
        if average:
            V = math.fsum(m[q].tolist()) if m is not None else float(count)
            want, bound = S / V, (2 * n + 2) * U * A / V
        else:
            want, bound = S, n * U * A
        err = abs(g[q] - want)
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, (tag, q, g[q], want, err, bound)
    return worst


@pytest.mark.parametrize("name", GRIDS)
def test_sums_on_all_dims_within_the_summation_bound(ocn, cases, name):
    c = cases[name]
    worst = 0.0
    for label, op in c.operands(("T", "u", "w", "w*u")):
        operand = D.operand_of(op, c.parents)
        for dims in ALL_DIMS:
            dd = (1, 2, 3) if dims is None else ((dims,) if isinstance(dims, int) else dims)
            mask, axes = ocn.diagnostics.dims_mask(dd), tuple(d - 1 for d in dd)
            plain = D.reduce_terms(c.grid, operand, mask, False)
            weighted = D.reduce_terms(c.grid, operand, mask, True)
            avg = ocn.Average(op, dims)
            assert avg.use_metric is (3 in dd and not c.grid.z_regular)
            checks = [("Average", ocn.Field(avg).interior(), weighted if avg.use_metric else plain, True, avg.use_metric),
                      ("Integral", ocn.Field(ocn.Integral(op, dims)).interior(), weighted, False, True),
                      ("Reduction sum", ocn.Field(ocn.Reduction("sum", op, dims)).interior(), plain, False, False)]
            if not hasattr(op, "interp_a"):
                s, mean = op.sum(dims=dims), op.mean(dims=dims)
                if dims is None:
                    assert isinstance(s, float) and isinstance(mean, float)
                    s, mean = np.full((1, 1, 1), s), np.full((1, 1, 1), mean)
                else:
                    assert s.loc == mean.loc == D_reduced(op.loc, dims)
                    s, mean = s.interior(), mean.interior()
                checks += [("sum", s, plain, False, False), ("mean", mean, plain, True, False)]
            for what, got, (terms, metric, count), average, with_metric in checks:
                assert got.shape == tuple(1 if d in axes else terms.shape[d] for d in range(3)), (name, label, dims, what)
                worst = max(worst, assert_sum_within_bound(got, terms, metric if with_metric else None, count, axes, average, (name, label, dims, what)))
    print(f"{name}: largest error / bound = {worst:.3f}")


def test_average_over_a_stretched_z_uses_the_metric(ocn, cases):
    T = cases["bpb_stretched"].fields["T"]
    a, m = ocn.Field(ocn.Average(T, dims=3)).interior(), T.mean(dims=3).interior()
    assert a.shape == m.shape == (70, 37, 1) and np.all(a != m)


# ---------------------------------------------------------------------------------------------------------------------
# reproducibility, status
# ---------------------------------------------------------------------------------------------------------------------
def test_the_same_compute_gives_the_same_bits(ocn, cases):
    c = cases["bpb_stretched"]
    for label, op in c.operands(("w*u", "T")):
        for dims in ((1, 2), None, 1, (1, 3)):
            f = ocn.Field(ocn.Average(op, dims))
            first = f.parent()
            for _ in range(3):
                assert np.array_equal(ocn.compute(f).parent(), first), (label, dims)
            assert np.array_equal(ocn.Field(ocn.Average(op, dims)).parent(), first)


def test_averages_of_ones_are_one_every_time(ocn, arch):
    """the reference's race test (test_field_scans.jl:254-279) at a size that takes no time"""
    grid = ocn.RectilinearGrid(arch, size=(96, 80, 12), x=(0, 2), y=(0, 2), z=(0, 2), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    c = ocn.CenterField(grid)
    c.set(1.0)
    avg = ocn.Field(ocn.Average(c, dims=(1, 2)))
    for _ in range(10):
        ocn.compute(avg)
        assert avg.interior().shape == (1, 1, 12) and np.all(avg.interior() == 1)


def test_compute_at_follows_the_status(ocn, arch):
    """test_field_scans.jl:323-349"""
    grid = ocn.RectilinearGrid(arch, size=(2, 2, 2), extent=(1, 1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    c = ocn.CenterField(grid)
    for dims in ALL_DIMS:
        avg = ocn.Field(ocn.Average(c, dims))
        assert avg.status is not None
        c.set(1.0)
        ocn.compute_at(avg, 1.0)                                  # will compute
        assert np.all(avg.interior() == 1) and avg.status.time == 1.0
        c.set(2.0)
        ocn.compute_at(avg, 1.0)                                  # will not: the status holds 1
        assert avg.status.time == 1.0 and np.all(avg.interior() == 1)
        ocn.compute_at(avg, 2.0)
        assert avg.status.time == 2.0 and np.all(avg.interior() == 2)


# ---------------------------------------------------------------------------------------------------------------------
# with a model
# ---------------------------------------------------------------------------------------------------------------------
def test_diagnostics_of_a_model_leave_it_untouched(ocn, arch):
    def make():
        grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        m = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T",))
        rng = np.random.default_rng(7)
        ocn.set_model(m, **{n: 0.1 * rng.standard_normal(m.grid.interior_size(f.loc)) for n, f in m.fields().items()})
        return m
    m, twin = make(), make()
    dt = 0.1 * m.grid.Δxᶜᵃᵃ / 0.6
    for model in (m, twin):
        for _ in range(2):
            ocn.time_step(model, dt)
    f = m.fields()
    before = {n: a.parent() for n, a in f.items()}
    parents = {f[n]: before[n] for n in f}
    for op, n in ((f["w"] * f["T"], 256), (f["u"], 256)):
        got = ocn.Field(ocn.Average(op, dims=(1, 2))).interior()
        terms, _, count = D.reduce_terms(m.grid, D.operand_of(op, parents), 3, False)
        assert count == n and got.shape == (1, 1, terms.shape[2])
        assert_sum_within_bound(got, terms, None, count, (0, 1), True, "model")
    for n, a in f.items():
        assert np.array_equal(a.parent(), before[n]), n
    for model in (m, twin):
        for _ in range(2):
            ocn.time_step(model, dt)
    for n, a in f.items():
        assert np.array_equal(a.parent(), twin.fields()[n].parent()), n


# ---------------------------------------------------------------------------------------------------------------------
# the raw C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_refuse_bad_arguments(ocn, arch, cases):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    c = cases["ppp"]
    T, u = c.fields["T"], c.fields["u"]
    out = ocn.Field(T.loc, c.grid)
    good = ocn.diagnostics.operand_struct(T)
    EINVAL = -1
    for mask in (0, 8, -1):
        assert L.ocn_reduce_operation(c.grid.handle, C.byref(good), 0, mask, 0, 0, out.data) == EINVAL
        assert b"dims_mask" in L.ocn_last_error()
    assert L.ocn_reduce_operation(c.grid.handle, C.byref(good), 4, 1, 0, 0, out.data) == EINVAL
    assert L.ocn_reduce_operation(c.grid.handle, C.byref(good), 1, 1, 1, 0, out.data) == EINVAL          # maximum takes no metric
    assert L.ocn_accumulate_operation(c.grid.handle, C.byref(good), 3, 0, 0, out.data) == EINVAL
    for call in (lambda: L.ocn_compute_operation(c.grid.handle, None, out.data), lambda: L.ocn_reduce_operation(c.grid.handle, None, 0, 1, 0, 0, out.data),
                 lambda: L.ocn_accumulate_operation(c.grid.handle, None, 0, 0, 0, out.data), lambda: L.ocn_compute_operation(c.grid.handle, C.byref(good), None),
                 lambda: L.ocn_compute_operation(None, C.byref(good), out.data)):
        assert call() == EINVAL and b"NULL" in L.ocn_last_error()
    bad = ocn.diagnostics.operand_struct(T * u)
    bad.loc[:] = [1, 0, 0]                                           # not the first field operand's location
    assert L.ocn_compute_operation(c.grid.handle, C.byref(bad), out.data) == EINVAL and b"location" in L.ocn_last_error()
    bad = ocn.diagnostics.operand_struct(T)
    bad.loc[:] = [0, 1, 0]
    assert L.ocn_reduce_operation(c.grid.handle, C.byref(bad), 0, 7, 0, 0, out.data) == EINVAL
    bad = ocn.diagnostics.operand_struct(T)
    bad.op = 9
    assert L.ocn_compute_operation(c.grid.handle, C.byref(bad), out.data) == EINVAL
    bad = ocn.diagnostics.operand_struct(2 / T)
    bad.b = None                                                     # no field operand at all
    assert L.ocn_compute_operation(c.grid.handle, C.byref(bad), out.data) == EINVAL
    ocn.synchronize()
    assert not out.parent().any()                                    # nothing was launched
    # a connected (partitioned) grid handle is refused by the library itself, whatever the host layer does
    part = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    c, pout = ocn.Field(T.loc, part), ocn.Field(T.loc, part)
    operand = _lib.Operand()
    operand.op, operand.a = 0, c.data
    ENOTSUP = -2
    for call in (lambda: L.ocn_compute_operation(part.handle, C.byref(operand), pout.data), lambda: L.ocn_reduce_operation(part.handle, C.byref(operand), 0, 3, 0, 0, pout.data),
                 lambda: L.ocn_accumulate_operation(part.handle, C.byref(operand), 2, 0, 0, pout.data)):
        assert call() == ENOTSUP and b"partitioned" in L.ocn_last_error()
