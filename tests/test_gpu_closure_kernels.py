"""The closure kernels of csrc/ocn_closures.h where the other files leave them open: the eddy-coefficient kernels (AnisotropicMinimumDissipation,
Smagorinsky) at the edges of the 63 columns x 4 rows x z-chunk tile of their marching forms -- marching == per-cell == the oracle / the numpy
restatement, every tracer count -- and the error codes of the four stand-alone closure-tendency entry points on invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from helpers import tanh_faces
import immersed_cases as IC
import smagorinsky_reference as R

pytestmark = pytest.mark.gpu

OCN_OK, OCN_EINVAL, OCN_ENOTSUP = 0, -1, -2          # include/ocn_mi355x.h

# a marching block writes 63 columns (one wave) and 4 rows, and walks a chunk of at least min(Nz, 8) levels
GRIDS = {
    "ppp_63x5x9": dict(size=(63, 5, 9), topology="PPP", stretched=False),         # exactly one wave's columns, one row more than a block
    "ppb_64x3x20": dict(size=(64, 3, 20), topology="PPB", stretched=True),        # one column in a second wave, fewer rows than a block, chunks of 8, 8, 4
    "bbb_127x4x8": dict(size=(127, 4, 8), topology="BBB", stretched=False),       # a third wave of one column
}
CKAPPA = [1 / 3, 1 / 12, 0.2, 0.5]


def _z_of(c):
    return tanh_faces(c["size"][2]) if c["stretched"] else ((-1.0, 0.0) if c["topology"][2] == "B" else (0.0, 1.0))


def _grid(ocn, arch, name):
    c = GRIDS[name]
    topo = tuple({"P": ocn.Periodic, "B": ocn.Bounded}[t] for t in c["topology"])
    return ocn.RectilinearGrid(arch, size=c["size"], x=(0.0, 1.0), y=(0.0, 1.0), z=_z_of(c), topology=topo, halo=(3, 3, 3))


def _interior(grid, a):
    return a[grid.Hx:grid.Hx + grid.Nx, grid.Hy:grid.Hy + grid.Ny, grid.Hz:grid.Hz + grid.Nz]


# ---------------------------------------------------------------------------------------------------------------------
# AnisotropicMinimumDissipation: νₑ and every κₑ
# ---------------------------------------------------------------------------------------------------------------------
_amd_cache = {}


def _amd_oracle(oracle, name, ntr):
    """the oracle model of a grid with `ntr` tracers in a random state after update_state: parent arrays of u, v, w, the tracers (halos
    filled) and of nu_e, kappa_e* (halos filled). Computed once per (grid, ntr) and left unchanged."""
    if (name, ntr) not in _amd_cache:
        c = GRIDS[name]
        g = oracle.Grid(c["size"], topology=tuple({"P": 0, "B": 1}[t] for t in c["topology"]), x=(0.0, 1.0), y=(0.0, 1.0), z=_z_of(c))
        m = oracle.Model(g, ntr)
        m.set_amd(Cnu=1 / 3, Ckappa=CKAPPA[:ntr] if ntr else 1 / 3)
        rng = np.random.default_rng(8 + ntr)
        names = m.names()
        m.set(enforce_incompressibility=False, **{n: rng.standard_normal(g.interior(m.field(n), m.loc(n)).shape) for n in names})
        m.update_state(False)
        fields = {n: m.field(n).copy(order="F") for n in names}
        coeffs = [m.field("nu_e").copy(order="F")] + [m.field("kappa_e%d" % t).copy(order="F") for t in range(ntr)]
        for a in list(fields.values()) + coeffs:
            a.setflags(write=False)
        _amd_cache[(name, ntr)] = (fields, coeffs)
    return _amd_cache[(name, ntr)]


def _amd_fields(ocn, grid, parents):
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    out = []
    for n, a in parents.items():
        f = make.get(n, ocn.CenterField)(grid)
        f.set_parent(a)
        out.append(f)
    return out


def _amd_both(ocn, grid, flds, ntr, rng=None, fill=False):
    """νₑ, κₑ... by amd_march = 1 and 0 -> two lists of parent arrays"""
    names = tuple("c%d" % t for t in range(ntr))
    closure = ocn.AnisotropicMinimumDissipation(Cν=1 / 3, Cκ=dict(zip(names, CKAPPA)))
    outs = []
    try:
        for march in (1, 0):
            ocn.set_option("amd_march", march)
            nu, ka = ocn.CenterField(grid), [ocn.CenterField(grid) for _ in range(ntr)]
            ocn.kernels.compute_amd_diffusivities(grid, closure, names, flds, nu, ka, kernel_parameters=rng)
            if fill:
                ocn.fill_halo_regions([nu] + ka)
            outs.append([nu.parent()] + [k.parent() for k in ka])
    finally:
        ocn.set_option("amd_march", 1)
    return outs


@pytest.mark.parametrize("ntr", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", list(GRIDS))
def test_amd_diffusivities_at_tile_edges(ocn, oracle, arch, name, ntr):
    """amd_march = 1 == amd_march = 0 == the oracle model's nu_e / kappa_e* after update_state (halos filled), whole parent arrays; with four
    tracers both settings run the per-cell kernel (the marching kernel serves ntr <= 3)"""
    grid = _grid(ocn, arch, name)
    parents, want = _amd_oracle(oracle, name, ntr)
    flds = _amd_fields(ocn, grid, parents)
    march, cell = _amd_both(ocn, grid, flds, ntr, fill=True)
    assert len(march) == len(cell) == len(want) == 1 + ntr
    for q, (a, b, w) in enumerate(zip(march, cell, want)):
        assert w.max() > 0 and np.isfinite(w).all()
        assert np.array_equal(a, b), ("march != per-cell", q)
        assert np.array_equal(b, w), ("per-cell != oracle", q, np.abs(b - w).max())
        assert np.array_equal(a, w), ("march != oracle", q, np.abs(a - w).max())


def test_amd_diffusivities_on_a_range_into_the_halos(ocn, oracle, arch):
    """range = (0, Nx + 1, 0, Ny + 1, 1, Nz) on the triply periodic grid: the halo columns hold what the periodic fill would put there,
    nothing outside the range is written, and a range that reaches H cells into a halo is refused"""
    name, ntr = "ppp_63x5x9", 2
    grid = _grid(ocn, arch, name)
    parents, want = _amd_oracle(oracle, name, ntr)
    flds = _amd_fields(ocn, grid, parents)
    rng = (0, grid.Nx + 1, 0, grid.Ny + 1, 1, grid.Nz)
    H = grid.Hx
    sl = (slice(H - 1, H + grid.Nx + 1), slice(H - 1, H + grid.Ny + 1), slice(H, H + grid.Nz))
    march, cell = _amd_both(ocn, grid, flds, ntr, rng=rng)
    for a, b, w in zip(march, cell, want):
        assert np.array_equal(a, b)
        assert np.array_equal(a[sl], w[sl])
        a[sl] = 0.0
        assert not a.any()                                 # nothing outside the range is written
    from oldoceananigans_jl_amd import _lib
    names = ("c0", "c1")
    closure = ocn.AnisotropicMinimumDissipation(Cν=1 / 3, Cκ=dict(zip(names, CKAPPA)))
    for bad in ((1 - grid.Hx, grid.Nx, 1, grid.Ny, 1, grid.Nz), (1, grid.Nx, 1, grid.Ny + grid.Hy, 1, grid.Nz),
                (1, grid.Nx, 1, grid.Ny, 1 - grid.Hz, grid.Nz)):
        for march in (1, 0):
            ocn.set_option("amd_march", march)
            try:
                with pytest.raises(_lib.OcnError):
                    ocn.kernels.compute_amd_diffusivities(grid, closure, names, flds, ocn.CenterField(grid),
                                                          [ocn.CenterField(grid), ocn.CenterField(grid)], kernel_parameters=bad)
            finally:
                ocn.set_option("amd_march", 1)


# ---------------------------------------------------------------------------------------------------------------------
# Smagorinsky / SmagorinskyLilly: νₑ
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["constant", "lilly_seawater"])
@pytest.mark.parametrize("name", ["ppp_63x5x9", "ppb_64x3x20"])
def test_smagorinsky_viscosity_at_tile_edges(ocn, arch, name, variant):
    """smag_march = 1 == smag_march = 0 == the numpy restatement (tests/smagorinsky_reference.py)"""
    grid = _grid(ocn, arch, name)
    kind = "none" if variant == "constant" else "seawater"
    vals, _ = R.case_values(grid, kind)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    flds = {n: make.get(n, ocn.CenterField)(grid).set(v) for n, v in vals.items()}
    ocn.fill_halo_regions(list(flds.values()))
    P = {n: f.parent() for n, f in flds.items()}
    if variant == "constant":
        closure, buoyancy, Cb = ocn.Smagorinsky(coefficient=0.16), None, None
    else:
        closure, Cb = ocn.SmagorinskyLilly(C=0.16, Cb=1.0), 1.0
        buoyancy = ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=R.ALPHA, haline_contraction=R.BETA),
                                        gravitational_acceleration=R.GRAV)
    want = R.viscosity(R.Metrics(grid), P["u"], P["v"], P["w"], 0.16, Cb=Cb, buoyancy=R.buoyancy_of(kind, P))
    assert want.max() > 0 and np.isfinite(want).all()
    outs = []
    try:
        for march in (1, 0):
            ocn.set_option("smag_march", march)
            nu = ocn.CenterField(grid)
            ocn.kernels.compute_smagorinsky_viscosity(grid, closure, buoyancy, flds, flds["u"], flds["v"], flds["w"], nu)
            outs.append(nu.parent())
    finally:
        ocn.set_option("smag_march", 1)
    march, cell = outs
    assert np.array_equal(_interior(grid, cell), want), ("per-cell kernel", np.abs(_interior(grid, cell) - want).max())
    assert np.array_equal(_interior(grid, march), want), ("marching kernel", np.abs(_interior(grid, march) - want).max())
    assert np.array_equal(march, cell)                     # (halos: both leave the zeros of the allocation)


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone closure-tendency entry points on invalid arguments
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = ("plain", "vertically_implicit", "field", "smagorinsky")


def _call(ocn, entry, grid, nu=1e-3, kappa=1e-3, Pr=1.0, null=None):
    """one raw call of an entry point with u, v, w, one tracer and their tendencies on `grid` -> the return code. null: the name of an
    argument passed as NULL"""
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd.fields import _ptr_array
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField}
    f = {n: make.get(n, ocn.CenterField)(grid) for n in "uvwc"}
    G = {n: make.get(n, ocn.CenterField)(grid) for n in "uvwc"}
    nu_e = ocn.CenterField(grid)
    p = lambda n, x: None if null == n else x              # noqa: E731
    u, v, w = p("u", f["u"].data), p("v", f["v"].data), p("w", f["w"].data)
    tr, Gc = p("tracers", _ptr_array([f["c"]])), p("Gc", _ptr_array([G["c"]]))
    Gu, Gv, Gw = p("Gu", G["u"].data), p("Gv", G["v"].data), p("Gw", G["w"].data)
    one = lambda x: p("coefficients", (C.c_double * 1)(x))              # noqa: E731
    L = _lib.lib()
    if entry == "plain":
        return L.ocn_compute_closure_tendencies(grid.handle, u, v, w, tr, 1, nu, one(kappa), Gu, Gv, Gw, Gc, None)
    if entry == "vertically_implicit":
        return L.ocn_compute_closure_tendencies_vertically_implicit(grid.handle, u, v, w, tr, 1, nu, one(kappa), Gu, Gv, Gw, Gc, None)
    if entry == "field":
        return L.ocn_compute_closure_tendencies_field(grid.handle, u, v, w, tr, 1, p("nu_e", nu_e.data), p("coefficients", _ptr_array([nu_e])),
                                                      Gu, Gv, Gw, Gc, None)
    return L.ocn_compute_closure_tendencies_smagorinsky(grid.handle, u, v, w, tr, 1, p("nu_e", nu_e.data), one(Pr), Gu, Gv, Gw, Gc, None)


def test_closure_tendency_entry_points_refuse_invalid_arguments(ocn, arch):
    """the return codes of ocn_compute_closure_tendencies, _vertically_implicit, _field and _smagorinsky, recorded from the library before
    the closures moved into a header of their own"""
    B, P, Fl = ocn.Bounded, ocn.Periodic, ocn.Flat
    bounded = ocn.RectilinearGrid(arch, size=(8, 6, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B))
    periodic = ocn.RectilinearGrid(arch, size=(8, 6, 8), x=(0, 1), y=(0, 1), z=(0, 1), topology=(P, P, P))
    flat = ocn.RectilinearGrid(arch, size=(8, 1, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, Fl, B))
    immersed = IC.immersed_grid(ocn, arch, "G1")
    # valid calls first: the refusals below are not those of a broken set-up
    for entry in ENTRIES:
        assert _call(ocn, entry, bounded) == OCN_OK, entry
    for entry in ("plain", "field", "smagorinsky"):
        assert _call(ocn, entry, periodic) == OCN_OK, entry
    for entry in ("plain", "vertically_implicit"):
        assert _call(ocn, entry, flat) == OCN_OK, entry
    assert _call(ocn, "plain", immersed) == OCN_OK
    # NULL fields
    for entry in ENTRIES:
        for null in ("u", "v", "w", "Gu", "Gv", "Gw", "tracers", "Gc", "coefficients"):
            assert _call(ocn, entry, bounded, null=null) == OCN_EINVAL, (entry, null)
    for entry in ("field", "smagorinsky"):
        assert _call(ocn, entry, bounded, null="nu_e") == OCN_EINVAL, entry
    # negative ν (the entry points that take one)
    for entry in ("plain", "vertically_implicit"):
        assert _call(ocn, entry, bounded, nu=-1e-3) == OCN_EINVAL, entry
    # non-positive Pr
    for Pr in (0.0, -1.0, float("nan")):
        assert _call(ocn, "smagorinsky", bounded, Pr=Pr) == OCN_EINVAL, Pr
    # a Flat direction with coefficient arrays
    for entry in ("field", "smagorinsky"):
        assert _call(ocn, entry, flat) == OCN_ENOTSUP, entry
    # VerticallyImplicitTimeDiscretization on a grid that is not Bounded in z
    assert _call(ocn, "vertically_implicit", periodic) == OCN_EINVAL
    # each eddy or vertically implicit form on an immersed grid
    for entry in ("vertically_implicit", "field", "smagorinsky"):
        assert _call(ocn, entry, immersed) == OCN_ENOTSUP, entry
