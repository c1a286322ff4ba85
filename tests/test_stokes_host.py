"""CPU tests of stokes_drift = UniformStokesDrift: the descriptor against what the reference prints and evaluates (StokesDrifts.jl:89-123,
139-161), the refusals of the model constructor (all raised before a handle exists, on grids with architecture None), and the numpy
restatement (tests/stokes_reference.py) pinned independently of the kernels -- to exact products of uniform velocities, and to the two-point
averages of tests/tilted_reference.py, which tests/test_tilted_host.py pins to the oracle's exact f × U."""
import math
from collections import namedtuple

import numpy as np
import pytest

import stokes_reference as S
import tilted_reference as T
import vertically_implicit_reference as R
from helpers import tanh_faces


def _grid(ocn, size=(8, 6, 10), topology=("Periodic", "Periodic", "Bounded"), stretched=True):
    z = tanh_faces(size[-1]) if stretched else (-1.0, 0.0)
    kw = {d: (0.0, 1.0) for d, t in zip("xy", topology) if t != "Flat"}
    return ocn.RectilinearGrid(None, size=size, topology=tuple(getattr(ocn, t) for t in topology), z=z, **kw)


def _parents(m, seed, names="uvw"):
    r = np.random.default_rng(seed)
    shape = lambda n: tuple(m.N[d] + 2 * m.H[d] + (1 if (R.LOCS[n][d] == R.FACE and m.topo[d] == R.BOUNDED) else 0) for d in range(3))   # noqa: E731
    return {n: np.asfortranarray(r.standard_normal(shape(n))) for n in names}


def _tables(m, seed):
    r = np.random.default_rng(seed)
    Nz = m.N[2]
    return tuple(r.standard_normal(Nz + (1 if q in (1, 3) else 0)) for q in range(6))


# ---------------------------------------------------------------------------------------------------------------------
# the descriptor
# ---------------------------------------------------------------------------------------------------------------------
def test_summaries_of_the_docstring():
    """the two jldoctest outputs of StokesDrifts.jl:89-123, character for character"""
    import oldoceananigans_jl_amd as ocn

    def uniform_stokes_shear(z, t):
        return 0.005 * math.exp(z / 20)
    drift = ocn.UniformStokesDrift(**{"∂z_uˢ": uniform_stokes_shear})
    assert repr(drift) == ("UniformStokesDrift{Nothing}:\n"
                           "├── ∂z_uˢ: uniform_stokes_shear\n"
                           "├── ∂z_vˢ: zerofunction\n"
                           "├── ∂t_uˢ: zerofunction\n"
                           "└── ∂t_vˢ: zerofunction")
    assert drift.summary() == "UniformStokesDrift{Nothing}"

    def uniform_stokes_shear(z, t, p):                   # noqa: F811
        return p.uˢ * math.exp(z / p.h)
    P = namedtuple("P", ["uˢ", "h"])
    drift = ocn.UniformStokesDrift(dz_us=uniform_stokes_shear, parameters=P(0.005, 20))
    assert repr(drift) == ("UniformStokesDrift with parameters (uˢ=0.005, h=20):\n"
                           "├── ∂z_uˢ: uniform_stokes_shear\n"
                           "├── ∂z_vˢ: zerofunction\n"
                           "├── ∂t_uˢ: zerofunction\n"
                           "└── ∂t_vˢ: zerofunction")
    # a dictionary of parameters prints the same way
    assert ocn.UniformStokesDrift(parameters={"uˢ": 0.005, "h": 20}).summary() == "UniformStokesDrift with parameters (uˢ=0.005, h=20)"
    with pytest.raises(TypeError):
        ocn.UniformStokesDrift(dz_us=uniform_stokes_shear, **{"∂z_uˢ": uniform_stokes_shear})
    with pytest.raises(TypeError):
        ocn.UniformStokesDrift(dz_ws=uniform_stokes_shear)


def test_function_tables_are_evaluated_at_the_nodes_with_parameters_third():
    """∂z at znode(k, grid, Center()) and znode(k, grid, Face()), ∂t at the centres (StokesDrifts.jl:144-145,151-152,158-159); parameters is
    the third argument; numbers are constants, None is zero"""
    import oldoceananigans_jl_amd as ocn
    grid = _grid(ocn)
    Nz, Hz = grid.Nz, grid.Hz
    zc, zf = grid.zᵃᵃᶜ[Hz:Hz + Nz], grid.zᵃᵃᶠ[Hz:Hz + Nz + 1]
    assert np.array_equal(zc, grid.nodes((ocn.Center, ocn.Center, ocn.Center))[2].ravel())
    assert np.array_equal(zf, grid.nodes((ocn.Center, ocn.Center, ocn.Face))[2].ravel())
    seen = []

    def shear(z, t, p):
        seen.append((t, p))
        return 0.7 * math.exp(z / p)
    drift = ocn.UniformStokesDrift(dz_us=shear, dz_vs=None, dt_us=0.25, dt_vs=lambda z, t, p: 0.02 * (1 + z), parameters=0.3)
    dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c = drift.tables(grid, 0.0)
    assert all(s == (0.0, 0.3) for s in seen) and len(seen) == 2 * Nz + 1
    assert np.array_equal(dzu_c, [0.7 * math.exp(z / 0.3) for z in zc]) and np.array_equal(dzu_f, [0.7 * math.exp(z / 0.3) for z in zf])
    assert dzv_c.shape == (Nz,) and dzv_f.shape == (Nz + 1,) and not dzv_c.any() and not dzv_f.any()
    assert np.array_equal(dtu_c, np.full(Nz, 0.25)) and np.array_equal(dtv_c, [0.02 * (1 + z) for z in zc])
    # without parameters the functions take (z, t)
    plain = ocn.UniformStokesDrift(dt_us=lambda z, t: z + t).tables(grid, 2.0)
    assert np.array_equal(plain[4], zc + 2.0)


def test_array_form_interpolates_the_face_array_to_the_centres():
    """UniformStokesDrift(grid; ∂z_uˢ = array on the z faces): the face table is the array, the centre table 0.5 (a[k] + a[k + 1])
    (StokesDrifts.jl:146-147,153-154); ∂t arrays are centre arrays (:160-161); the defaults are zero arrays; wrong lengths are ValueErrors"""
    import oldoceananigans_jl_amd as ocn
    grid = _grid(ocn)
    Nz = grid.Nz
    a = np.random.default_rng(1).standard_normal(Nz + 1)
    t = np.random.default_rng(2).standard_normal(Nz)
    drift = ocn.UniformStokesDrift(grid, dz_vs=a, dt_us=t)
    dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c = drift.tables(grid)
    assert np.array_equal(dzv_f, a) and np.array_equal(dzv_c, 0.5 * (a[:-1] + a[1:])) and np.array_equal(dtu_c, t)
    assert not dzu_c.any() and not dzu_f.any() and not dtv_c.any() and dzu_f.shape == (Nz + 1,)
    for kw in (dict(dz_us=np.zeros(Nz)), dict(dz_vs=np.zeros(Nz + 2)), dict(dt_us=np.zeros(Nz + 1)), dict(dt_vs=np.zeros(3))):
        with pytest.raises(ValueError, match="values"):
            ocn.NonhydrostaticModel(grid=grid, stokes_drift=ocn.UniformStokesDrift(grid, **kw))
    with pytest.raises(ValueError, match="one-dimensional"):
        ocn.UniformStokesDrift(grid, dz_us=np.zeros((Nz + 1, 2)))


def test_refusals_before_any_handle():
    """StokesDrift by name; a partitioned grid; a Flat z; time dependence -- all on grid metadata, so this runs without a GPU"""
    import oldoceananigans_jl_amd as ocn
    grid = _grid(ocn)
    drift = ocn.UniformStokesDrift(dz_us=lambda z, t: 0.7 * math.exp(z / 0.3))
    with pytest.raises(NotImplementedError, match="StokesDrift"):
        ocn.NonhydrostaticModel(grid=grid, stokes_drift=ocn.StokesDrift(**{"∂z_uˢ": lambda x, y, z, t: z}))
    with pytest.raises(NotImplementedError, match="UniformStokesDrift"):
        ocn.NonhydrostaticModel(grid=grid, stokes_drift="waves")

    class Partitioned:                                     # what DistributedRectilinearGrid looks like to the model: a `local` grid
        local = grid
        halo_size = grid.halo_size
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=Partitioned(), stokes_drift=drift)
    flat = ocn.RectilinearGrid(None, size=(8, 8), extent=(1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Flat))
    with pytest.raises(NotImplementedError, match="Flat"):
        ocn.NonhydrostaticModel(grid=flat, stokes_drift=drift)
    with pytest.raises(NotImplementedError, match="time dependence"):
        ocn.NonhydrostaticModel(grid=grid, stokes_drift=ocn.UniformStokesDrift(dt_us=lambda z, t: math.exp(z) * math.cos(t)))


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ocn_mi355x.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _lib.lib()
    for s in ("ocn_add_stokes_drift", "ocn_model_set_stokes_drift"):
        assert s + "(" in header and s in _lib.SYMBOLS and hasattr(lib, s)
        assert f"(:{s}, libocn)" in integration
    for key in ("stokes_drift", "stokes_path"):
        assert '"' + key + '"' in header
    assert callable(ocn.kernels.add_stokes_drift)
    for name in ("UniformStokesDrift", "StokesDrift"):
        assert name in ocn.__all__, name


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, pinned independently of the kernels
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "ppb_stretched": dict(size=(8, 6, 10), topology=("Periodic", "Periodic", "Bounded"), stretched=True),
    "pfb": dict(size=(8, 8), topology=("Periodic", "Flat", "Bounded"), stretched=False),
    "bbb": dict(size=(12, 10, 8), topology=("Bounded", "Bounded", "Bounded"), stretched=False),
    "ppp": dict(size=(8, 8, 8), topology=("Periodic", "Periodic", "Periodic"), stretched=False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_uniform_velocities_give_exact_products(name):
    """w ≡ W: every average is W exactly, so G_u gains W * ∂z_uˢ(z_c[k]) and G_v W * ∂z_vˢ(z_c[k]) -- one rounding, the product's; u ≡ U₀ (v
    ≡ 0) gives G_w = -U₀ * ∂z_uˢ(z_f[k]) and v ≡ V₀ (u ≡ 0) G_w = -V₀ * ∂z_vˢ(z_f[k]); with G = 0 and no ∂t the sums add zeros. This pins signs,
    tables and levels on something the kernels and the restatement do not share."""
    import oldoceananigans_jl_amd as ocn
    m = R.Metrics.of_grid(_grid(ocn, **CASES[name]))
    dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c = tables = _tables(m, 4)
    zeros = lambda: {n: np.zeros_like(a) for n, a in _parents(m, 0).items()}       # noqa: E731
    W, U0, V0 = 1.7, -0.9, 2.3
    U = zeros()
    U["w"][...] = W
    G = S.add_stokes_drift(m, tables[:4] + (np.zeros_like(dtu_c), np.zeros_like(dtv_c)), U, zeros())
    for n, tab in (("u", dzu_c), ("v", dzv_c)):
        r = m.default_range(R.LOCS[n], True)
        got = R._Window(m, r)(G[n])
        assert got.size and np.all(got == (W * tab)[None, None, r[4] - 1:r[5]]), (name, n)
    assert not G["w"].any()
    for vel, val, tab in (("u", U0, dzu_f), ("v", V0, dzv_f)):
        U = zeros()
        U[vel][...] = val
        G = S.add_stokes_drift(m, tables, U, zeros())
        r = m.default_range(R.LOCS["w"], True)
        got = R._Window(m, r)(G["w"])
        assert r[4] == (2 if m.topo[2] == R.BOUNDED else 1) and np.all(got == (-val * tab)[None, None, r[4] - 1:r[5]]), (name, vel)
        # w ≡ 0: G_u and G_v hold 0 * table + ∂t = the ∂t tables
        ru = m.default_range(R.LOCS["u"], True)
        assert np.all(R._Window(m, ru)(G["u"]) == dtu_c[None, None, ru[4] - 1:ru[5]])
        rv = m.default_range(R.LOCS["v"], True)
        assert np.all(R._Window(m, rv)(G["v"]) == dtv_c[None, None, rv[4] - 1:rv[5]])


@pytest.mark.parametrize("name", list(CASES))
def test_averages_are_those_of_the_tilted_restatement(name):
    """ℑxᶠᵃᵃ and ℑyᵃᶠᵃ of this file == x_dot_g_b / y_dot_g_b of tilted_reference with ĝ = 1 (the product by 1 is exact); ℑxᶜᵃᵃ, ℑyᵃᶜᵃ and
    ℑzᵃᵃᶜ are tilted_reference's own functions. With tables of ones the curls are the composed averages: x_curl == ½ (ℑx w[k] + ℑx w[k + 1]),
    z_curl == -½ (ℑxᶜ u[k - 1] + ℑxᶜ u[k]) - ½ (ℑyᶜ v[k - 1] + ℑyᶜ v[k])."""
    import oldoceananigans_jl_amd as ocn
    m = R.Metrics.of_grid(_grid(ocn, **CASES[name]))
    U = _parents(m, 5)
    Nz = m.N[2]
    ones = tuple(np.ones(Nz + (1 if q in (1, 3) else 0)) for q in range(6))
    up = lambda r, dk: r[:4] + (r[4] + dk, r[5] + dk)                                # noqa: E731
    r = m.default_range(R.LOCS["u"], True)
    W = R._Window(m, r)
    assert np.array_equal(S._Ix_f(m, W, U["w"], (0, 0, 0)), T.x_dot_g_b(m, 1.0, U["w"], r))
    assert np.array_equal(S.x_curl(m, ones, U, r), 0.5 * (T.x_dot_g_b(m, 1.0, U["w"], r) + T.x_dot_g_b(m, 1.0, U["w"], up(r, 1))))
    r = m.default_range(R.LOCS["v"], True)
    W = R._Window(m, r)
    assert np.array_equal(S._Iy_f(m, W, U["w"], (0, 0, 0)), T.y_dot_g_b(m, 1.0, U["w"], r))
    assert np.array_equal(S.y_curl(m, ones, U, r), 0.5 * (T.y_dot_g_b(m, 1.0, U["w"], r) + T.y_dot_g_b(m, 1.0, U["w"], up(r, 1))))
    r = m.default_range(R.LOCS["w"], True)
    W = R._Window(m, r)
    ua = 0.5 * (T._Ix_c(m, W, U["u"], (0, 0, -1)) + T._Ix_c(m, W, U["u"], (0, 0, 0)))
    va = 0.5 * (T._Iy_c(m, W, U["v"], (0, 0, -1)) + T._Iy_c(m, W, U["v"], (0, 0, 0)))
    assert np.array_equal(S.z_curl(m, ones, U, r), (-ua) - va)
    if m.flat[1]:                                         # the Flat identity: ℑyᵃᶠᵃ w is w itself
        assert np.array_equal(S._Iy_f(m, W, U["w"], (0, 0, 0)), W(U["w"]))


@pytest.mark.parametrize("name", list(CASES))
def test_zero_tables_change_nothing_and_ranges_are_kept(name):
    """tables of zeros: every tendency np.array_equal to its input (G + w * 0 + 0); random tables over a trimmed range: entries outside it
    keep their bits, entries inside change"""
    import oldoceananigans_jl_amd as ocn
    m = R.Metrics.of_grid(_grid(ocn, **CASES[name]))
    U, G0 = _parents(m, 6), _parents(m, 7)
    Nz = m.N[2]
    zero = tuple(np.zeros(Nz + (1 if q in (1, 3) else 0)) for q in range(6))
    G = S.add_stokes_drift(m, zero, U, {n: a.copy(order="F") for n, a in G0.items()})
    for n in "uvw":
        assert np.array_equal(G[n], G0[n]), (name, n)
    tables = _tables(m, 8)
    for rng in (None, (2, 7, 1, 1, 3, 7) if m.flat[1] else (2, 7, 2, 5, 3, 7)):
        G = S.add_stokes_drift(m, tables, U, {n: a.copy(order="F") for n, a in G0.items()}, rng=rng)
        for n in "uvw":
            r = m.default_range(R.LOCS[n], True) if rng is None else rng
            inside = np.zeros(G[n].shape, dtype=bool)
            R._Window(m, r)(inside)[...] = True
            changed = G[n] != G0[n]
            assert changed[inside].all() and not changed[~inside].any(), (name, n, rng)
