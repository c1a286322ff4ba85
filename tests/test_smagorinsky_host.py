"""CPU tests of the Smagorinsky / SmagorinskyLilly closures: analytic known answers of the numpy restatement (tests/smagorinsky_reference.py)
that the GPU kernels are compared with bit for bit, the regime condition of the random-state cases used on the GPU, and the host mirror
(constructors, reprs, refusals, Pr handling, halo requirement). No device."""
import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn

import smagorinsky_reference as R

F, Cn = ocn.Face, ocn.Center
LOCS = {"u": (F, Cn, Cn), "v": (Cn, F, Cn), "w": (Cn, Cn, F), "b": (Cn, Cn, Cn)}


def _grid(spacing):
    L = 6.0 * spacing
    return ocn.RectilinearGrid(None, size=(6, 6, 6), x=(0.0, L), y=(0.0, L), z=(-L, 0.0), topology=(ocn.Bounded,) * 3, halo=(3, 3, 3))


def _parent(grid, name, fn):
    """fn(x, y, z) at every node of the field's parent array (halos included: no fill is involved)"""
    lx, ly, lz = LOCS[name]
    x = (grid.xᶠᵃᵃ if lx is F else grid.xᶜᵃᵃ)[:, None, None]
    y = (grid.yᵃᶠᵃ if ly is F else grid.yᵃᶜᵃ)[None, :, None]
    z = (grid.zᵃᵃᶠ if lz is F else grid.zᵃᵃᶜ)[None, None, :]
    return np.asfortranarray(np.broadcast_to(fn(x, y, z), grid.total_size(LOCS[name])).astype(np.float64))


INNER = (2, 5, 2, 5, 2, 5)          # cells whose stencils stay inside the analytic fields


@pytest.mark.parametrize("spacing", [1.0, 2.0])
def test_known_answers_of_the_restatement(spacing):
    """cbrt(1) and cbrt(8) are exact: Δf² = spacing²"""
    g = _grid(spacing)
    m = R.Metrics(g)
    assert np.all(m.df2 == spacing * spacing)
    C, df2 = 0.16, spacing * spacing
    zero = lambda name: _parent(g, name, lambda x, y, z: 0.0 * (x + y + z))          # noqa: E731
    # u = S z: Σ13 = S / 2, Σ² = S² / 2, νₑ = C² Δf² |S|
    for S in (0.7, -1.3):
        u = _parent(g, "u", lambda x, y, z: S * z + 0.0 * (x + y))
        nu = R.viscosity(m, u, zero("v"), zero("w"), C, rng=INNER)
        assert np.allclose(nu, C * C * df2 * abs(S), rtol=1e-13, atol=0.0)
    # u = (x, y, -2 z): Σ² = 1 + 1 + 4, νₑ = C² Δf² sqrt(12)
    u = _parent(g, "u", lambda x, y, z: x + 0.0 * (y + z))
    v = _parent(g, "v", lambda x, y, z: y + 0.0 * (x + z))
    w = _parent(g, "w", lambda x, y, z: -2.0 * z + 0.0 * (x + y))
    for Cb in (None, 1.0):
        nu = R.viscosity(m, u, v, w, C, Cb=Cb, rng=INNER)
        assert np.allclose(nu, C * C * df2 * np.sqrt(12.0), rtol=1e-13, atol=0.0)
    # fluid at rest: exactly +0.0 and no NaN anywhere, with every coefficient and buoyancy
    b = _parent(g, "b", lambda x, y, z: 0.3 * z + 0.0 * (x + y))
    for Cb, buoy in ((None, None), (1.0, None), (1.0, ("tracer", b)), (0.5, ("seawater", b, b, 9.8, 2e-4, 8e-4))):
        nu = R.viscosity(m, zero("u"), zero("v"), zero("w"), C, Cb=Cb, buoyancy=buoy, rng=(0, 7, 0, 7, 0, 7))
        assert not np.isnan(nu).any() and np.all(nu == 0.0) and not np.signbit(nu).any()
    # b = N² z under u = S z with Cb = 1: νₑ = C² Δf² |S| sqrt(1 - 2 N² / S²)
    S = 1.1
    u = _parent(g, "u", lambda x, y, z: S * z + 0.0 * (x + y))
    unstratified = R.viscosity(m, u, zero("v"), zero("w"), C, Cb=1.0, buoyancy=None, rng=INNER)
    assert np.allclose(unstratified, C * C * df2 * S, rtol=1e-13, atol=0.0)
    for N2 in (0.1, 0.4):
        b = _parent(g, "b", lambda x, y, z: N2 * z + 0.0 * (x + y))
        nu = R.viscosity(m, u, zero("v"), zero("w"), C, Cb=1.0, buoyancy=("tracer", b), rng=INNER)
        assert np.allclose(nu, C * C * df2 * S * np.sqrt(1 - 2 * N2 / (S * S)), rtol=1e-13, atol=0.0)
        # the same through SeawaterBuoyancy: b = g (α T - β S) with T = b / (g α), S = 0
        T = _parent(g, "b", lambda x, y, z: N2 / (9.8 * 2e-4) * z + 0.0 * (x + y))
        nu = R.viscosity(m, u, zero("v"), zero("w"), C, Cb=1.0, buoyancy=("seawater", T, zero("b"), 9.8, 2e-4, 8e-4), rng=INNER)
        assert np.allclose(nu, C * C * df2 * S * np.sqrt(1 - 2 * N2 / (S * S)), rtol=1e-12, atol=0.0)       # (N² itself is rounded here)
    # N² >= S² / 2: exactly 0
    for N2 in (S * S, 5.0):
        b = _parent(g, "b", lambda x, y, z: N2 * z + 0.0 * (x + y))
        assert np.all(R.viscosity(m, u, zero("v"), zero("w"), C, Cb=1.0, buoyancy=("tracer", b), rng=INNER) == 0.0)
    # N² < 0: the unstratified value, bit for bit
    b = _parent(g, "b", lambda x, y, z: -0.8 * z + 0.0 * (x + y))
    assert np.array_equal(R.viscosity(m, u, zero("v"), zero("w"), C, Cb=1.0, buoyancy=("tracer", b), rng=INNER), unstratified)


def test_tracer_flux_divergence_of_the_restatement():
    """c = x² / 2 with uniform νₑ = 1: q = -(x / Pr), ∇·q = -1 / Pr; νₑ = z with c = z²/2: ∇·q = -(2 z) / Pr"""
    g = _grid(1.0)
    m = R.Metrics(g)
    c = _parent(g, "b", lambda x, y, z: 0.5 * x * x + 0.0 * (y + z))
    one = _parent(g, "b", lambda x, y, z: 1.0 + 0.0 * (x + y + z))
    for Pr in (1.0, 2.0, 3.0):
        assert np.allclose(R.div_q(m, c, one, Pr, rng=INNER), -1.0 / Pr, rtol=1e-13, atol=0.0)
    c = _parent(g, "b", lambda x, y, z: 0.5 * z * z + 0.0 * (x + y))
    nu = _parent(g, "b", lambda x, y, z: -z + 0.0 * (x + y))
    zc = g.zᵃᵃᶜ[g.Hz + 1:g.Hz + 5][None, None, :]
    assert np.allclose(R.div_q(m, c, nu, 3.0, rng=INNER), np.broadcast_to((2 * zc) / 3.0, (4, 4, 4)), rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("kind,Cb", [c for c in R.LILLY_CASES if c[0] != "none"])
@pytest.mark.parametrize("name", list(R.GRIDS))
def test_random_state_cases_reach_every_regime(oracle, name, kind, Cb):
    """the inputs of the GPU parity cases: at least 10 % of the cells with ς = 1, with 0 < ς < 1 and with ς = 0"""
    grid = R.make_grid(ocn, None, name)
    vals, _ = R.case_values(grid, kind)
    P = R.oracle_parents(oracle, name, vals)
    fr = R.regime_fractions(R.Metrics(grid), P["u"], P["v"], P["w"], Cb, R.buoyancy_of(kind, P))
    print(name, kind, Cb, fr)
    assert min(fr) >= 0.10, fr
    assert abs(sum(fr) - 1.0) < 1e-12


def test_constructors_reprs_and_refusals():
    s = ocn.Smagorinsky()
    assert (s.coefficient, s.Pr, s.lilly) == (0.16, 1.0, False)
    assert repr(s) == "Smagorinsky closure with coefficient = 0.16, Pr = 1.0"
    sl = ocn.SmagorinskyLilly()
    assert (sl.coefficient, sl.Cb, sl.Pr, sl.lilly) == (0.16, 1.0, 1.0, True)
    assert repr(sl) == "Smagorinsky closure with coefficient = LillyCoefficient(smagorinsky = 0.16, reduction_factor = 1.0), Pr = 1.0"
    assert ocn.SmagorinskyLilly(C=0.2, Cb=0.5, Pr=2).Cb == 0.5
    assert isinstance(sl, ocn.Smagorinsky)
    for bad in (lambda: ocn.Smagorinsky(coefficient=lambda x, y, z: 0.1), lambda: ocn.Smagorinsky(coefficient=ocn.DynamicCoefficient()),
                lambda: ocn.SmagorinskyLilly(C=ocn.DynamicCoefficient(averaging=1)), lambda: ocn.SmagorinskyLilly(Cb=lambda: 1),
                lambda: ocn.Smagorinsky(Pr=lambda: 1), lambda: ocn.Smagorinsky(Pr={"T": lambda: 1})):
        with pytest.raises(NotImplementedError):
            bad()
    with pytest.raises(ValueError):
        ocn.Smagorinsky(coefficient=-0.1)
    with pytest.raises(ValueError):
        ocn.Smagorinsky(Pr=0.0)
    with pytest.raises(ValueError):
        ocn.SmagorinskyLilly(Pr={"T": 1.0, "S": -2.0})


def test_prandtl_numbers_per_tracer():
    arr, _ = ocn.Smagorinsky(Pr=2).Pr_array(("T", "S"))
    assert arr.tolist() == [2.0, 2.0]
    arr, _ = ocn.SmagorinskyLilly(Pr={"S": 3, "T": 1}).Pr_array(("T", "S"))
    assert arr.tolist() == [1.0, 3.0]
    with pytest.raises(ValueError, match="missing"):
        ocn.Smagorinsky(Pr={"T": 1.0}).Pr_array(("T", "S"))
    arr, _ = ocn.Smagorinsky().Pr_array(())
    assert len(arr) == 1


def test_halo_requirement():
    """required_halo_size = 2 (AbstractScalarDiffusivity{TD, ThreeDimensionalFormulation, 2})"""
    for closure in (ocn.Smagorinsky(), ocn.SmagorinskyLilly()):
        assert ocn.required_halo_size_x(closure) == ocn.required_halo_size_y(closure) == ocn.required_halo_size_z(closure) == 2
    grid = ocn.RectilinearGrid(None, size=(4, 4, 4), extent=(1, 1, 1), halo=(1, 1, 1))
    from oldoceananigans_jl_amd.advection import inflate_halo_size
    assert inflate_halo_size(1, 1, 1, grid, ocn.Smagorinsky()) == (2, 2, 2)
    assert inflate_halo_size(1, 1, 1, grid, ocn.ScalarDiffusivity(ν=1)) == (1, 1, 1)
