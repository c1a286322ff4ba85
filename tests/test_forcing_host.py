"""CPU tests of the forcing mirror (oldoceananigans.jl_amd/forcings.py; reference src/Forcings/): the REPL output of the reference's
docstrings, the host tables ocn_model_set_forcing receives (evaluated at the forced field's nodes, halos included), MultipleForcings
regularisation and the refusals. No device: model_forcing works on grid metadata."""
import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn
from oldoceananigans_jl_amd import forcings as F

from helpers import tanh_faces

LOCS = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face),
        "T": (ocn.Center, ocn.Center, ocn.Center)}


def test_relaxation_docstrings():
    """relaxation.jl's jldoctests"""
    damping = ocn.Relaxation(rate=1 / 3600)
    assert repr(damping) == ("Relaxation{Float64, typeof(Oceananigans.Forcings.onefunction), typeof(Oceananigans.Forcings.zerofunction)}\n"
                             "├── rate: 0.0002777777777777778\n├── mask: 1\n└── target: 0")
    dTdz, T0, Lz = 0.001, 20, 100
    sponge = ocn.Relaxation(rate=1 / 60, target=ocn.LinearTarget["z"](intercept=T0, gradient=dTdz),
                            mask=ocn.GaussianMask["z"](center=-Lz, width=Lz / 4))
    assert repr(sponge) == ("Relaxation{Float64, GaussianMask{:z, Float64}, LinearTarget{:z, Float64}}\n"
                            "├── rate: 0.016666666666666666\n├── mask: exp(-(z + 100.0)^2 / (2 * 25.0^2))\n└── target: 20.0 + 0.001 * z")
    assert sponge.summary() == "Relaxation(rate=0.016666666666666666, mask=exp(-(z + 100.0)^2 / (2 * 25.0^2)), target=20.0 + 0.001 * z)"
    assert repr(ocn.GaussianMask["z"](center=0, width=1)) == "GaussianMask{:z, Int64}(0, 1)"
    assert ocn.GaussianMask("x", center=0, width=1).summary() == "exp(-x^2 / (2 * 1^2))"
    assert ocn.GaussianMask("y", center=0.5, width=2.0).summary() == "exp(-(y - 0.5)^2 / (2 * 2.0^2))"
    mask = ocn.PiecewiseLinearMask["z"](center=0, width=1)
    assert repr(mask) == "PiecewiseLinearMask{:z, Int64}(0, 1)"
    assert mask(0.0) == 1 and mask(1.0) == mask(-1.0) == 0
    assert mask.summary() == "piecewise_linear(z, center=0, width=1)"
    assert ocn.LinearTarget["z"](intercept=0, gradient=1e-6).summary() == "0.0 + 1.0e-6 * z"
    mf = ocn.MultipleForcings(damping, sponge)
    assert repr(mf) == ("MultipleForcings with 2 forcings:\n├ Relaxation(rate=0.0002777777777777778, mask=1, target=0)\n"
                        "└ " + sponge.summary())


@pytest.mark.parametrize("stretched", [False, True])
def test_tables_at_the_field_nodes(stretched):
    z = tanh_faces(6) if stretched else (-1.0, 0.0)
    grid = ocn.RectilinearGrid(None, size=(8, 5, 6), x=(0.0, 2.0), y=(-1.0, 1.0), z=z,
                               topology=(ocn.Periodic, ocn.Bounded, ocn.Bounded), halo=(3, 3, 3))
    nodes = {("x", ocn.Face): grid.xᶠᵃᵃ, ("x", ocn.Center): grid.xᶜᵃᵃ, ("y", ocn.Face): grid.yᵃᶠᵃ, ("y", ocn.Center): grid.yᵃᶜᵃ,
             ("z", ocn.Face): grid.zᵃᵃᶠ, ("z", ocn.Center): grid.zᵃᵃᶜ}
    rate = 1 / 7
    for name, loc in LOCS.items():
        for d, D in enumerate("xyz"):
            mask = ocn.GaussianMask(D, center=0.1, width=0.3)
            target = ocn.LinearTarget(D, intercept=2, gradient=0.5)
            (t,) = F.model_forcing(grid, LOCS, {name: ocn.Relaxation(rate=rate, mask=mask, target=target)})[name]
            xi = np.asarray(nodes[(D, loc[d])])
            assert t.kind == 2 and t.mask_dir == d and t.target_dir == d
            assert len(t.mask_table) == grid.total_size(loc)[d] == len(xi)
            assert np.array_equal(t.mask_table, rate * np.exp(-((xi - 0.1) * (xi - 0.1)) / (2 * (0.3 * 0.3))))
            assert np.array_equal(t.target_table, 2.0 + 0.5 * xi)
            # element H + ξ - 1 is node ξ: the interior nodes of Field.nodes
            H = grid.halo_size[d]
            interior = grid.nodes(loc)[d].ravel()
            assert np.array_equal(t.target_table[H:H + len(interior)], 2.0 + 0.5 * interior)
        (t,) = F.model_forcing(grid, LOCS, {name: ocn.Relaxation(rate=rate, mask=ocn.PiecewiseLinearMask("z", center=-0.5, width=0.25),
                                                                   target=3)})[name]
        zi = np.asarray(nodes[("z", loc[2])])
        assert np.array_equal(t.mask_table, rate * np.maximum(0.0, 1.0 - np.abs(zi + 0.5) / 0.25))
        assert t.target_dir == -1 and t.target == 3.0
    (t,) = F.model_forcing(grid, LOCS, {"T": ocn.Relaxation(rate=0.25)})["T"]
    assert (t.mask_dir, t.rate_mask, t.target_dir, t.target) == (-1, 0.25, -1, 0.0)


def test_multiple_forcings_equivalence():
    grid = ocn.RectilinearGrid(None, size=(4, 4, 4), extent=(1, 1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    a = ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask["z"](center=-0.5, width=0.1))
    b = np.arange(64.0).reshape(4, 4, 4)
    forms = [(a, b), ocn.MultipleForcings(a, b), ocn.MultipleForcings((a, b)), [a, ocn.Forcing(b)]]
    got = [F.model_forcing(grid, LOCS, {"T": f})["T"] for f in forms]
    for terms in got:
        assert [t.kind for t in terms] == [2, 1]
        assert np.array_equal(terms[0].mask_table, got[0][0].mask_table)
        assert np.array_equal(terms[1].array, b)
    # host twin of the device sum: N <= 4 left to right, N > 4 from zero
    phi = np.random.default_rng(0).standard_normal((4, 4, 4))
    two = F.evaluate(got[0], grid, LOCS["T"], phi)
    one_a = F.evaluate(got[0][:1], grid, LOCS["T"], phi)
    assert np.array_equal(two, one_a + b)
    five = F.evaluate([got[0][1]] * 5, grid, LOCS["T"], phi)
    assert np.array_equal(five, ((((0.0 + b) + b) + b) + b) + b)


def test_zero_target_keeps_the_sign_of_zero():
    grid = ocn.RectilinearGrid(None, size=(4, 4, 4), extent=(1, 1, 1))
    (t,) = F.model_forcing(grid, LOCS, {"T": ocn.Relaxation(rate=2.0)})["T"]
    out = F.evaluate([t], grid, LOCS["T"], np.zeros((4, 4, 4)))
    assert np.all(out == 0) and not np.any(np.signbit(out))           # 2 * (0 - (+0.0)) = +0.0


def test_refusals():
    grid = ocn.RectilinearGrid(None, size=(4, 4), extent=(1, 1), topology=(ocn.Periodic, ocn.Flat, ocn.Bounded))
    locs = dict(LOCS)
    with pytest.raises(NotImplementedError, match="callable"):
        F.model_forcing(grid, locs, {"T": lambda x, y, z, t: 1.0})
    with pytest.raises(NotImplementedError, match="ContinuousForcing"):
        F.model_forcing(grid, locs, {"T": ocn.Forcing(lambda x, y, z, t: 1.0)})
    with pytest.raises(NotImplementedError, match="DiscreteForcing"):
        F.model_forcing(grid, locs, {"T": ocn.Forcing(lambda i, j, k, g, c, f: 1.0, discrete_form=True)})
    with pytest.raises(NotImplementedError, match="AdvectiveForcing"):
        F.model_forcing(grid, locs, {"T": ocn.AdvectiveForcing(w=1.0)})

    class FieldTimeSeries:
        pass
    with pytest.raises(NotImplementedError, match="FieldTimeSeries"):
        F.model_forcing(grid, locs, {"T": FieldTimeSeries()})
    with pytest.raises(NotImplementedError, match="not a velocity or tracer"):
        F.model_forcing(grid, locs, {"b": ocn.Relaxation(rate=1.0)})
    with pytest.raises(ValueError, match="Flat"):
        F.model_forcing(grid, locs, {"T": ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask["y"](center=0, width=1))})
    with pytest.raises(ValueError, match="Flat"):
        F.model_forcing(grid, locs, {"T": ocn.Relaxation(rate=1.0, target=ocn.LinearTarget["y"](intercept=0, gradient=1))})
    with pytest.raises(ValueError, match="size"):
        F.model_forcing(grid, locs, {"T": np.zeros((3, 1, 4))})
    with pytest.raises(ValueError, match="at most"):
        F.model_forcing(grid, locs, {"T": (ocn.Relaxation(rate=1.0),) * 9})
    # a mask along a non-Flat direction of the same grid is fine
    assert len(F.model_forcing(grid, locs, {"T": ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask["x"](center=0, width=1))})["T"]) == 1


def test_model_constructor_refuses_before_any_device_work():
    """the constructor regularises the forcing before it creates the library handle: a refused forcing needs no GPU"""
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    with pytest.raises(NotImplementedError, match="callable"):
        ocn.NonhydrostaticModel(grid=grid, forcing={"u": lambda x, y, z, t: 0.0})
    with pytest.raises(NotImplementedError, match="not a velocity or tracer"):
        ocn.NonhydrostaticModel(grid=grid, tracers=("T",), forcing={"S": ocn.Relaxation(rate=1.0)})
