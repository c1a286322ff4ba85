"""CPU tests of background_fields (oldoceananigans.jl_amd/background_fields.py; reference Models/NonhydrostaticModels/background_fields.jl):
the numpy restatement of advection with separate advecting and advected fields (tests/background_reference.py) pinned to the oracle bit
for bit, the orchestrated yardstick with all-zero backgrounds pinned to the oracle's own model, the host regularisation (analytic halos,
accepted forms, refusals -- on grid metadata, no device) and the new C ABI symbols."""
import ctypes as C

import numpy as np
import pytest

import background_reference as B
import vertically_implicit_reference as R
from helpers import tanh_faces

# PPP, PPB stretched, BBB (wall fall-backs of both interpolations), (Periodic, Flat, Bounded), a two-cell direction (WENO{2} along y and the
# Centered(order = 2) transports of the fluxes that point along it), and a launch range
CASES = {
    "ppp": ((16, 16, 16), (0, 0, 0), False, None),
    "ppb_stretched": ((16, 16, 12), (0, 0, 1), True, None),
    "bbb": ((12, 10, 8), (1, 1, 1), False, None),
    "pfb": ((18, 1, 8), (0, 3, 1), False, None),
    "two_cell_y": ((16, 2, 8), (0, 0, 1), False, None),
    "ppb_range": ((16, 16, 12), (0, 0, 1), True, (3, 14, 2, 9, 2, 11)),
}


def _oracle_grid(O, size, topo, stretched):
    z = tanh_faces(size[2]) if stretched else ((-1.0, 0.0) if topo[2] == 1 else (0.0, 1.0))
    return O.Grid(size, topology=topo, x=(0.0, 1.0), y=(0.0, 1.0), z=z)


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_is_the_oracle_when_advecting_is_advected(oracle, case):
    """random fields over the whole parent arrays: -div(U, u|v|w) == oro_compute_Gu/Gv/Gw and -div(U, c) == oro_compute_Gc, np.array_equal"""
    size, topo, stretched, rng = CASES[case]
    g = _oracle_grid(oracle, size, topo, stretched)
    m = R.Metrics.of_oracle(g)
    r = np.random.default_rng(5)
    P = {n: np.asfortranarray(r.standard_normal(g.parent_size(R.LOCS[n]))) for n in "uvwc"}
    for n in "uvwc":
        want = g.zeros(R.LOCS[n])
        g.compute_G(n, P["u"], P["v"], P["w"], want, c=P["c"] if n == "c" else None, rng=rng)
        got = B.advective_tendency(m, n, (P["u"], P["v"], P["w"]), P[n], rng=rng)
        assert np.abs(want).max() > 1.0
        assert np.array_equal(got, want), (n, np.abs(got - want).max())
        # accumulate: G - div on a pre-filled array, entries outside the range untouched
        G0 = np.asfortranarray(r.standard_normal(want.shape))
        acc = B.advective_tendency(m, n, (P["u"], P["v"], P["w"]), P[n], rng=rng, G=G0.copy(order="F"), accumulate=True)
        div, rr = B.advective_divergence(m, n, (P["u"], P["v"], P["w"]), P[n], rng)
        inside = np.zeros(want.shape, dtype=bool)
        B._window(m, inside, rr)[...] = True
        assert inside.any() and np.array_equal(acc[~inside], G0[~inside])
        assert np.array_equal(B._window(m, acc, rr), B._window(m, G0, rr) - div)
        assert np.array_equal(B._window(m, want, rr), -div + 0.0)


def test_fma_is_one_rounding():
    from fractions import Fraction
    r = np.random.default_rng(0)
    a, b = r.standard_normal(4000), r.standard_normal(4000)
    c = -a * b * (1 + 1e-16 * r.standard_normal(4000))          # heavy cancellation: the product's low part decides the result
    got = B.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert not np.array_equal(a * b + c, want)


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_orchestrated_yardstick_with_zero_backgrounds_is_the_oracle_model(oracle, timestepper):
    """every background an explicit all-zero array (so both terms and the totals are evaluated): two steps == the oracle's own model with
    the same closure in u, v, w, the tracers and p (±0 compare equal, nothing else may differ)"""
    O = oracle
    size, topo = (8, 8, 8), (0, 0, 1)
    g = O.Grid(size, topology=topo, x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(8))
    nu, kappa = 2e-3, (5e-3, 1e-3)
    mo = O.Model(g, 2)
    mo.set_closure(nu=nu, kappa=kappa)
    names = ["u", "v", "w", "c0", "c1"]
    zeros = {n: g.zeros(R.LOCS.get(n, R.LOCS["c"])) for n in names}
    yard = B.BackgroundOrchestrated(O, g, 2, nu, kappa, background=zeros, closure="oracle")
    r = np.random.default_rng(11)
    vals = {n: 0.3 * r.standard_normal(g.interior(zeros[n], R.LOCS.get(n, R.LOCS["c"])).shape) for n in names}
    mo.set(**vals)
    yard.set(**vals)
    dt = 0.01
    for _ in range(2):
        if timestepper == "RungeKutta3":
            mo.time_step(dt)
            yard.time_step(dt)
        else:
            mo.time_step_ab2(dt)
            yard.time_step_ab2(dt)
    for n in names:
        assert np.all(np.isfinite(yard.U[n]))
        assert np.array_equal(yard.U[n], mo.field(n)), (n, np.abs(yard.U[n] - mo.field(n)).max())
    assert np.array_equal(yard.p, mo.field("p"))
    assert yard.time == mo.time and yard.iteration == 2


# ---------------------------------------------------------------------------------------------------------------------
# regularisation: on grid metadata only (RectilinearGrid(None, ...)), nothing touches a device
# ---------------------------------------------------------------------------------------------------------------------
def _host_grid(ocn, topology=None):
    topology = topology or (ocn.Periodic, ocn.Periodic, ocn.Bounded)
    return ocn.RectilinearGrid(None, size=(8, 6, 4), x=(0.0, 2.0), y=(-1.0, 1.0), z=(-1.0, 0.0), topology=topology)


def test_function_halos_are_the_analytic_continuation():
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import background_fields as BF
    grid = _host_grid(ocn)
    bg = BF.regularize_background_fields({"b": lambda x, y, z: x + 0 * y + 0 * z, "u": lambda x, y, z, t: x + 0 * y + 0 * z}, ("b", "c"), grid)
    dx = grid.Δxᶜᵃᵃ
    b = bg.tracers.b
    assert b.shape == grid.total_size((ocn.Center,) * 3) == (14, 12, 10) and bg.tracers.c is None and bg.velocities.v is None
    # x₀ - Δx/2, x₀ - 3Δx/2, ... beyond the Periodic edge and Lx + Δx/2, ... beyond the other: never the periodic wrap
    want = grid.x0 + dx * (np.arange(14) - 3 + 0.5)
    assert np.allclose(b[:, 0, 0], want, rtol=0, atol=1e-15) and np.array_equal(b[:, 0, 0], grid.xᶜᵃᵃ)
    assert b[2, 5, 5] == -0.125 and b[2, 5, 5] != b[2 + 8, 5, 5] and b[11, 0, 0] == 2.125
    assert np.all(b == b[:, :1, :1])
    u = bg.velocities.u                                 # at Face in x: the face nodes, halos included
    assert np.array_equal(u[:, 3, 3], grid.xᶠᵃᵃ) and u[0, 0, 0] == -0.75
    # z on a Bounded direction: beyond the wall likewise, w at faces has Nz + 1 + 2 Hz points
    w = BF.regularize_background_fields({"w": lambda x, y, z: z + 0 * x + 0 * y}, (), grid).velocities.w
    assert w.shape == (14, 12, 11) and np.array_equal(w[4, 4, :], grid.zᵃᵃᶠ) and w[0, 0, 0] == -1.75


def test_accepted_forms():
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import background_fields as BF
    grid = _host_grid(ocn)
    ccc, fcc = (ocn.Center,) * 3, (ocn.Face, ocn.Center, ocn.Center)
    shape = grid.total_size(ccc)
    N2 = 1e-4
    field = ocn.Field(fcc, grid, data=C.c_void_p(8))               # a view of foreign memory: never dereferenced on the host
    arr = np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
    bg = BF.regularize_background_fields(
        ocn.BackgroundFields(b=ocn.BackgroundField(lambda x, y, z, t, p: p["N2"] * z + 0 * x + 0 * y, parameters={"N2": N2}),
                             c=ocn.BackgroundField(2.5), d=3, e=arr, u=field), ("b", "c", "d", "e", "f"), grid)
    assert np.array_equal(bg.tracers.b[0, 0, :], N2 * grid.zᵃᵃᶜ)
    assert bg.tracers.c.shape == shape and np.all(bg.tracers.c == 2.5) and np.all(bg.tracers.d == 3.0)
    assert np.array_equal(bg.tracers.e, arr) and bg.tracers.e.flags.f_contiguous
    assert bg.velocities.u is field and bg.tracers.f is None and bg.velocities.w is None
    assert BF.regularize_background_fields(None, ("b",), grid) is None and BF.regularize_background_fields({}, ("b",), grid) is None
    assert "BackgroundField" in ocn.__all__ and "BackgroundFields" in ocn.__all__


def test_refusals():
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import background_fields as BF
    grid = _host_grid(ocn)
    ccc = (ocn.Center,) * 3
    wrong = ocn.Field(ccc, grid, data=C.c_void_p(8))
    with pytest.raises(ValueError, match=r"Cannot use field at \(Center, Center, Center\) as a background field at \(Face, Center, Center\)"):
        BF.regularize_background_fields({"u": wrong}, ("b",), grid)
    with pytest.raises(ValueError, match="not a velocity or tracer"):
        BF.regularize_background_fields({"T": 1.0}, ("b",), grid)
    with pytest.raises(NotImplementedError, match="time dependence"):
        BF.regularize_background_fields({"b": lambda x, y, z, t: z * np.exp(t) + 0 * x + 0 * y}, ("b",), grid)
    with pytest.raises(NotImplementedError, match="background_closure_fluxes"):
        BF.regularize_background_fields(ocn.BackgroundFields(background_closure_fluxes=True, b=1.0), ("b",), grid)
    with pytest.raises(ValueError, match="parent size"):
        BF.regularize_background_fields({"b": np.zeros((8, 6, 4))}, ("b",), grid)

    class Partitioned:                                     # what DistributedRectilinearGrid looks like to the model: a `local` grid
        local = grid
    with pytest.raises(NotImplementedError, match="partitioned"):
        BF.regularize_background_fields({"b": 1.0}, ("b",), Partitioned())
    # the model constructor regularises before it creates the library handle: a refused background needs no GPU
    with pytest.raises(ValueError, match="not a velocity or tracer"):
        ocn.NonhydrostaticModel(grid=ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1)), tracers=("b",), background_fields={"T": 1.0})
    with pytest.raises(NotImplementedError, match="time dependence"):
        ocn.NonhydrostaticModel(grid=ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1)), tracers=("b",),
                                background_fields={"u": lambda x, y, z, t: t + 0 * x + 0 * y + 0 * z})


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ocn_mi355x.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _lib.lib()
    for s in ("ocn_compute_advective_tendency", "ocn_sum_parent", "ocn_model_set_background_field"):
        assert s + "(" in header and s in _lib.SYMBOLS and hasattr(lib, s)
        assert f"(:{s}, libocn)" in integration
    for key in ("background_fields", "background_tendency_path", "bg_<name>", "total_u"):
        assert key in header
    assert callable(ocn.kernels.compute_advective_tendency) and callable(ocn.kernels.sum_parent)
    assert "Background fields are not stored" in ocn.checkpointer.__doc__
