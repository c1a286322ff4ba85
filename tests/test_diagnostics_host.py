"""CPU tests of the diagnostics: the numpy restatement (tests/diagnostics_reference.py) pinned to the numbers the reference's tests and
docstrings print (test/test_field_scans.jl:172-216,245-251; metric_field_reductions.jl:112-142,171-204; Fields/scans.jl:126-197) and to
the interpolation formulas written out by hand, and the host logic of oldoceananigans_jl_amd/diagnostics.py (locations, dims, reduced
sizes, refusals) on grids with architecture None and borrowed fields, so nothing touches a device."""
import ctypes as C
import math

import numpy as np
import pytest

import diagnostics_reference as D
import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import diagnostics
from helpers import tanh_faces

CCC = (ocn.Center, ocn.Center, ocn.Center)
FCC = (ocn.Face, ocn.Center, ocn.Center)
CFC = (ocn.Center, ocn.Face, ocn.Center)
CCF = (ocn.Center, ocn.Center, ocn.Face)
FFF = (ocn.Face, ocn.Face, ocn.Face)
PPB = (ocn.Periodic, ocn.Periodic, ocn.Bounded)


def host_field(grid, loc, parents, value=None, seed=None):
    """a borrowed field (no device memory) and its host parent array: f(x, y, z) over the interior, or seeded noise everywhere"""
    f = ocn.Field(loc, grid, data=C.c_void_p(0))
    if value is not None:
        a = np.zeros(f.shape, order="F")
        x, y, z = grid.nodes(loc)
        a[f._interior_slices()] = value(x, y, z)
    else:
        a = np.asfortranarray(0.5 + np.random.default_rng(seed).standard_normal(f.shape))
    parents[f] = a
    return f


def scan_value(scan, parents):
    return D.evaluate_scan(scan, parents)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's numbers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretched", [False, True])
def test_field_scans_numbers(stretched):
    """test/test_field_scans.jl:172-216,245-251 on the 2 x 2 x 2 grid with trilinear(x, y, z) = x + y + z, z regular and z = [0, 1, 2];
    every partial sum is a small dyadic number, so `==`"""
    grid = ocn.RectilinearGrid(None, size=(2, 2, 2), x=(0, 2), y=(0, 2), z=np.array([0.0, 1.0, 2.0]) if stretched else (0, 2), topology=PPB)
    assert grid.z_regular is (not stretched)
    P = {}
    tri = lambda x, y, z: x + y + z                                  # noqa: E731
    T, w = host_field(grid, CCC, P, tri), host_field(grid, CCF, P, tri)
    assert ocn.Average(T).use_metric is stretched and ocn.Average(T, dims=(1, 2)).use_metric is False
    Txyz, Txy, Tx = (scan_value(ocn.Average(T, dims=d), P) for d in (None, (1, 2), 1))
    assert Txyz.shape == (1, 1, 1) and Txyz[0, 0, 0] == 3
    assert np.array_equal(Txy[0, 0, :], [2.5, 3.5])
    assert np.array_equal(Tx[0], [[2, 3], [3, 4]])
    wxyz, wxy, wx = (scan_value(ocn.Average(w, dims=d), P) for d in (None, (1, 2), 1))
    assert wxyz[0, 0, 0] == 3
    assert np.array_equal(wxy[0, 0, :], [2, 3, 4])
    assert np.array_equal(wx[0], [[1.5, 2.5, 3.5], [2.5, 3.5, 4.5]])
    for f in (T, w):
        assert np.array_equal(scan_value(ocn.Integral(f, dims=1), P), 2 * scan_value(ocn.Average(f, dims=1), P))
        assert np.array_equal(scan_value(ocn.Integral(f, dims=(1, 2)), P), 4 * scan_value(ocn.Average(f, dims=(1, 2)), P))
    cum = lambda f, d, r=False: scan_value(ocn.CumulativeIntegral(f, dims=d, reverse=r), P)       # noqa: E731
    assert np.array_equal(cum(T, 1)[:, 0, 0], [1.5, 4]) and np.array_equal(cum(T, 2)[0, :, 0], [1.5, 4])
    assert np.array_equal(cum(T, 3)[0, 0, :], [1.5, 4])
    assert np.array_equal(cum(T, 1, True)[:, 0, 0], [4, 2.5]) and np.array_equal(cum(T, 3, True)[0, 0, :], [4, 2.5])
    assert np.array_equal(cum(w, 1)[:, 0, 0], [1, 3]) and np.array_equal(cum(w, 2)[0, :, 0], [1, 3])
    assert np.array_equal(cum(w, 3)[0, 0, :], [1, 3, 6])
    assert np.array_equal(cum(w, 1, True)[:, 0, 0], [3, 2]) and np.array_equal(cum(w, 3, True)[0, 0, :], [6, 5, 3])
    for d, at in ((1, np.s_[:, 0, 0]), (2, np.s_[0, :, 0]), (3, np.s_[0, 0, :])):
        assert np.array_equal(cum(2 * T, d)[at], [3, 8])
        assert np.array_equal(cum(2 * T, d, True)[at], [8, 5])


def test_docstring_numbers():
    # Integral of x y z over the unit cube on 8^3 (metric_field_reductions.jl:112-142): 0.125 within n 2^-53 Σ|x|
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), x=(0, 1), y=(0, 1), z=(0, 1), topology=PPB)
    P = {}
    f = host_field(grid, CCC, P, lambda x, y, z: x * y * z)
    terms, _, n = D.reduce_terms(grid, D.operand_of(f, P), 7, True)
    value = scan_value(ocn.Integral(f), P)[0, 0, 0]
    assert n == 512 and abs(value - 0.125) <= n * 2.0 ** -53 * math.fsum(np.abs(terms).ravel())
    # CumulativeIntegral of z on (Flat, Flat, Bounded), 8 cells (:171-204): C[1, 1, 8] = 0.5, max = 0.5, min = 0.0078125
    grid = ocn.RectilinearGrid(None, size=8, z=(0, 1), topology=(ocn.Flat, ocn.Flat, ocn.Bounded))
    c = host_field(grid, CCC, P, lambda x, y, z: z + 0 * x + 0 * y)
    Cz = scan_value(ocn.CumulativeIntegral(c, dims=3), P)
    assert Cz.shape == (1, 1, 8) and Cz[0, 0, 7] == 0.5 and Cz.max() == 0.5 and Cz.min() == 0.0078125
    # maximum! and cumsum! of c^2, c = x + y + z on 3^3 (scans.jl:126-197), to the six printed digits
    grid = ocn.RectilinearGrid(None, size=(3, 3, 3), x=(0, 1), y=(0, 1), z=(0, 1), topology=(ocn.Periodic,) * 3)
    c = host_field(grid, CCC, P, lambda x, y, z: x + y + z)
    digits = np.vectorize(lambda v: float(f"{v:.6g}"))
    mx = scan_value(ocn.Reduction("maximum", c ** 2, dims=3), P)
    assert np.array_equal(digits(mx[:, :, 0]), [[1.36111, 2.25, 3.36111], [2.25, 3.36111, 4.69444], [3.36111, 4.69444, 6.25]])
    cs = scan_value(ocn.Accumulation("cumsum", c ** 2, dims=3), P)
    table = [[[0.25, 0.694444, 1.36111], [0.694444, 1.36111, 2.25], [1.36111, 2.25, 3.36111]],
             [[0.944444, 2.05556, 3.61111], [2.05556, 3.61111, 5.61111], [3.61111, 5.61111, 8.05556]],
             [[2.30556, 4.30556, 6.97222], [4.30556, 6.97222, 10.3056], [6.97222, 10.3056, 14.3056]]]
    for k in range(3):
        assert np.array_equal(digits(cs[:, :, k]), table[k])


# ---------------------------------------------------------------------------------------------------------------------
# locations and interpolation
# ---------------------------------------------------------------------------------------------------------------------
def _bpb(stretched=True):
    return ocn.RectilinearGrid(None, size=(6, 5, 4), x=(0, 1), y=(0, 1), z=tanh_faces(4) if stretched else (-1, 0),
                               topology=(ocn.Bounded, ocn.Periodic, ocn.Bounded))


def test_locations_and_interpolation_formulas():
    grid = _bpb()
    P = {}
    u, w, T, q = (host_field(grid, loc, P, seed=s) for s, loc in enumerate((FCC, CCF, CCC, FFF)))
    H = grid.halo_size
    at = lambda f, i, j, k: P[f][i - 1 + H[0], j - 1 + H[1], k - 1 + H[2]]          # noqa: E731  the reference's 1-based index
    # w * u at (Center, Center, Face): u interpolated z of x (ℑxzᶜᵃᶠ = ℑzᵃᵃᶠ of ℑxᶜᵃᵃ)
    op = w * u
    assert op.location == CCF and op.interp_a == "identity" and op.interp_b == "ℑxzᶜᵃᶠ"
    val = D.compute_operation(grid, D.operand_of(op, P))
    assert val.shape == grid.interior_size(CCF) == (6, 5, 5)
    for i, j, k in ((1, 1, 1), (6, 5, 5), (3, 2, 4)):
        ux = lambda kk: 0.5 * (at(u, i, j, kk) + at(u, i + 1, j, kk))               # noqa: E731
        assert val[i - 1, j - 1, k - 1] == at(w, i, j, k) * (0.5 * (ux(k - 1) + ux(k)))
    # u * w at (Face, Center, Center): ℑxzᶠᵃᶜ
    op = u * w
    assert op.location == FCC and op.interp_b == "ℑxzᶠᵃᶜ"
    val = D.compute_operation(grid, D.operand_of(op, P))
    assert val.shape == (7, 5, 4)
    for i, j, k in ((1, 1, 1), (7, 5, 4), (4, 3, 2)):
        wx = lambda kk: 0.5 * (at(w, i - 1, j, kk) + at(w, i, j, kk))               # noqa: E731
        assert val[i - 1, j - 1, k - 1] == at(u, i, j, k) * (0.5 * (wx(k) + wx(k + 1)))
    # T * u: ℑxᶜᵃᵃ; a number; a square; three directions nest x of y of z
    op = T * u
    assert op.location == CCC and op.interp_b == "ℑxᶜᵃᵃ"
    val = D.compute_operation(grid, D.operand_of(op, P))
    assert val[2, 1, 3] == at(T, 3, 2, 4) * (0.5 * (at(u, 3, 2, 4) + at(u, 4, 2, 4)))
    op = 0.5 * u
    assert op.location == FCC and op.a == 0.5 and op.b is u
    assert np.array_equal(D.compute_operation(grid, D.operand_of(op, P)), 0.5 * P[u][3:-3, 3:-3, 3:-3])
    op = u ** 2
    assert op.op == "*" and op.a is u and op.b is u and op.interp_b == "identity"
    assert np.array_equal(D.compute_operation(grid, D.operand_of(op, P)), P[u][3:-3, 3:-3, 3:-3] ** 2)
    op = T - q
    assert op.interp_b == "ℑxyzᶜᶜᶜ"
    val = D.compute_operation(grid, D.operand_of(op, P))
    i, j, k = 2, 5, 3
    Z = lambda ii, jj: 0.5 * (at(q, ii, jj, k) + at(q, ii, jj, k + 1))              # noqa: E731
    Y = lambda ii: 0.5 * (Z(ii, j) + Z(ii, j + 1))                                  # noqa: E731
    assert val[i - 1, j - 1, k - 1] == at(T, i, j, k) - 0.5 * (Y(i) + Y(i + 1))
    for other in (2.0 / T, T / 2, 1 + T, T + 1, 1 - T):
        assert other.location == CCC


def test_flat_direction_interpolates_by_identity():
    grid = ocn.RectilinearGrid(None, size=(6, 4), x=(0, 1), z=(-1, 0), topology=(ocn.Bounded, ocn.Flat, ocn.Bounded))
    P = {}
    T, v = host_field(grid, CCC, P, seed=1), host_field(grid, CFC, P, seed=2)
    assert v.shape == T.shape == (12, 1, 10)
    val = D.compute_operation(grid, D.operand_of(T * v, P))
    assert np.array_equal(val, (P[T] * P[v])[3:-3, :, 3:-3])
    # the metric of a Flat direction is 1
    assert np.array_equal(scan_value(ocn.Integral(T, dims=2), P), P[T][3:-3, :, 3:-3])


def test_metrics_at_the_operands_location():
    grid = _bpb()
    dzc, dzf = grid.Δzᵃᵃᶜ[3:3 + 4], grid.Δzᵃᵃᶠ[3:3 + 5]
    dx, dy = grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ
    assert np.array_equal(D.metric(grid, CCC, 4).ravel(), dzc) and np.array_equal(D.metric(grid, CCF, 4).ravel(), dzf)
    assert D.metric(grid, CCC, 1).ravel() == dx and D.metric(grid, CCC, 2).ravel() == dy and D.metric(grid, CCC, 3).ravel() == dx * dy
    assert np.array_equal(D.metric(grid, CCF, 5).ravel(), dx * dzf) and np.array_equal(D.metric(grid, CCC, 6).ravel(), dy * dzc)
    assert np.array_equal(D.metric(grid, CCF, 7).ravel(), (dx * dy) * dzf)
    # Average over the stretched z differs from the plain mean and equals Σ T Δz / Σ Δz
    P = {}
    T = host_field(grid, CCC, P, seed=3)
    Ti = P[T][3:-3, 3:-3, 3:-3]
    avg = scan_value(ocn.Average(T, dims=3), P)
    assert avg.shape == (6, 5, 1)
    assert np.allclose(avg[:, :, 0], (Ti * dzc).sum(axis=2) / dzc.sum(), rtol=1e-14)
    assert not np.allclose(avg[:, :, 0], Ti.mean(axis=2), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# dims, reduced locations and sizes, refusals, the existing call forms
# ---------------------------------------------------------------------------------------------------------------------
def test_dims_and_reduced_sizes():
    grid = _bpb()
    P = {}
    u = host_field(grid, FCC, P, seed=1)
    assert ocn.Average(u).dims == (1, 2, 3) and ocn.Average(u, dims=2).dims == (2,) and ocn.Integral(u, dims=(3, 1)).dims == (1, 3)
    for dims, loc, total, interior in (((1,), (None, ocn.Center, ocn.Center), (1, 11, 10), (1, 5, 4)),
                                       ((2,), (ocn.Face, None, ocn.Center), (13, 1, 10), (7, 1, 4)),
                                       ((3,), (ocn.Face, ocn.Center, None), (13, 11, 1), (7, 5, 1)),
                                       ((1, 2), (None, None, ocn.Center), (1, 1, 10), (1, 1, 4)),
                                       ((1, 3), (None, ocn.Center, None), (1, 11, 1), (1, 5, 1)),
                                       ((2, 3), (ocn.Face, None, None), (13, 1, 1), (7, 1, 1)),
                                       ((1, 2, 3), (None, None, None), (1, 1, 1), (1, 1, 1))):
        scan = ocn.Reduction("sum", u, dims)
        assert scan.location == loc and grid.total_size(loc) == total and grid.interior_size(loc) == interior
        assert scan_value(scan, P).shape == interior
        # all N + 1 points of a Face field on a Bounded direction count
        assert D.reduce_terms(grid, D.operand_of(u, P), diagnostics.dims_mask(dims), False)[2] == int(np.prod([(7, 5, 4)[d - 1] for d in dims]))
    assert ocn.CumulativeIntegral(u, dims=1).location == FCC and ocn.Accumulation("cumsum", u * u, dims=3, reverse=True).reverse
    reduced = ocn.Field((None, None, ocn.Center), grid, data=C.c_void_p(0))
    assert reduced.shape == (1, 1, 10) and reduced._interior_slices() == (slice(0, 1), slice(0, 1), slice(3, 7))
    for bad in (0, 4, (1, 1), (), "x", 1.5):
        with pytest.raises((ValueError, TypeError)):
            ocn.Average(u, dims=bad)
    for bad in ((1, 2), None, 0):
        with pytest.raises(ValueError):
            ocn.CumulativeIntegral(u, dims=bad)


def test_refusals():
    grid, other = _bpb(), _bpb()
    P = {}
    u, T = host_field(grid, FCC, P, seed=1), host_field(grid, CCC, P, seed=2)
    with pytest.raises(ValueError, match="different grids"):
        u * host_field(other, CCC, P, seed=3)
    for make in (lambda: (u * T) * T, lambda: T + (u * T), lambda: 2 * (u * T), lambda: (u * T) ** 2, lambda: ocn.Average(ocn.Average(T, dims=1)),
                 lambda: T * ocn.Integral(T, dims=1)):
        with pytest.raises(NotImplementedError, match=r"Field\((op|scan)\)"):
            make()
    for exponent in (3, 0.5, -1, True):
        with pytest.raises(NotImplementedError, match="exponent"):
            u ** exponent
    for kw in ({"condition": lambda *a: True}, {"mask": 0}):
        for make in (lambda kw=kw: ocn.Average(T, **kw), lambda kw=kw: ocn.Integral(T, dims=1, **kw), lambda kw=kw: ocn.CumulativeIntegral(T, 3, **kw),
                     lambda kw=kw: ocn.Reduction("sum", T, 1, **kw), lambda kw=kw: ocn.Accumulation("cumsum", T, 1, **kw),
                     lambda kw=kw: T.sum(**kw), lambda kw=kw: T.mean(dims=1, **kw), lambda kw=kw: T.maximum(**kw), lambda kw=kw: diagnostics.minimum(T, **kw)):
            with pytest.raises(NotImplementedError, match=list(kw)[0]):
                make()
    for operand in (np.sin, "∂x(u)", np.ones(3)):                      # derivative and unary operands, functions
        with pytest.raises(NotImplementedError):
            ocn.Average(operand)
        with pytest.raises(NotImplementedError):
            T * operand
    reduced = ocn.Field((None, None, ocn.Center), grid, data=C.c_void_p(0))
    for make in (lambda: ocn.Average(reduced), lambda: reduced * 2, lambda: T * reduced):
        with pytest.raises(NotImplementedError, match="reduced field"):
            make()
    with pytest.raises(NotImplementedError):
        ocn.Reduction("prod", T, 1)
    with pytest.raises(NotImplementedError):
        ocn.Accumulation("cumprod", T, 1)
    with pytest.raises(NotImplementedError):
        T.maximum(f=np.square)
    # a partitioned (connected) grid: refused by name before any device call
    part = ocn.RectilinearGrid(None, size=(6, 5, 4), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    c = ocn.Field(CCC, part, data=C.c_void_p(0))
    for make in (lambda: ocn.Average(c), lambda: c * 2, lambda: c.sum(), lambda: ocn.CumulativeIntegral(c, 3)):
        with pytest.raises(NotImplementedError, match="partitioned"):
            make()
    # nothing above reached the library: it is not even initialised here
    with pytest.raises(TypeError):
        ocn.Field(3.0)


def test_existing_field_call_forms_and_exports():
    grid = _bpb()
    f = ocn.Field(FCC, grid, data=C.c_void_p(0))
    assert f.loc == FCC and f.shape == (13, 11, 10) and f.operand is None and f.status is None and not f._owns
    g = ocn.Field(FCC, grid, C.c_void_p(16))
    assert g.data.value == 16 and g.loc_codes == (1, 0, 0)
    assert ocn.compute(f) is f                                           # compute! of a plain field does nothing
    for name in ("Average", "Integral", "CumulativeIntegral", "Reduction", "Accumulation", "BinaryOperation", "compute", "compute_at", "FieldStatus"):
        assert name in ocn.__all__
    for name in ("sum", "mean", "maximum", "minimum"):                   # would shadow builtins under `import *`
        assert name not in ocn.__all__ and callable(getattr(diagnostics, name))
