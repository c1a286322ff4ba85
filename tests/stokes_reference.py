"""Numpy restatement of the terms of a UniformStokesDrift (test infrastructure), every expression with the line of the reference it restates:

  * x_curl / y_curl / z_curl  -- x_curl_Uˢ_cross_U = ℑxzᶠᵃᶜ(w) ∂z_uˢ(z_c), y_curl_Uˢ_cross_U = ℑyzᵃᶠᶜ(w) ∂z_vˢ(z_c), z_curl_Uˢ_cross_U =
                                 (-ℑxzᶜᵃᶠ(u)) ∂z_uˢ(z_f) - ℑyzᵃᶜᶠ(v) ∂z_vˢ(z_f) (StokesDrifts.jl:170-178) with ℑxzᶠᵃᶜ = ℑzᵃᵃᶜ(ℑxᶠᵃᵃ ·) and so on
                                 (Operators/interpolation_operators.jl:8-15,50-56), the identity along a Flat direction (:87-112)
  * add_stokes_drift          -- G_u = (G_u + x_curl) + ∂t_uˢ, G_v = (G_v + y_curl) + ∂t_vˢ, G_w = (G_w + z_curl) + 0
                                 (nonhydrostatic_tendency_kernel_functions.jl:100-101,162-163,226-227; ∂t_wˢ = zero(grid), StokesDrifts.jl:168)
  * StokesOrchestrated        -- tilted_reference.TiltedOrchestrated whose update_state! inserts the terms after the closure term and before
                                 the forcing, the order of the reference's tendency functions

The oracle has no Stokes drift; tests/test_stokes_host.py pins this file to exact products of uniform velocities and to the two-point
averages of tests/tilted_reference.py. `tables` = (dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c): per level, index k - 1; the centre tables have
Nz values, the face tables Nz + 1. Every operation is an elementwise IEEE float64 operation in the stated association order. Arrays are
PARENT arrays, Fortran order, indexed [i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]."""
import numpy as np

import tilted_reference as T
from tilted_reference import _Ix_c, _Iy_c, _empty, _ranges
from vertically_implicit_reference import _Window


def _Ix_f(m, W, a, o):       # ℑxᶠᵃᵃ: (a[i - 1] + a[i]) / 2 (interpolation_operators.jl:9)
    return W(a, *o) if m.flat[0] else 0.5 * (W(a, o[0] - 1, o[1], o[2]) + W(a, *o))


def _Iy_f(m, W, a, o):       # ℑyᵃᶠᵃ: (a[j - 1] + a[j]) / 2 (:12)
    return W(a, *o) if m.flat[1] else 0.5 * (W(a, o[0], o[1] - 1, o[2]) + W(a, *o))


def _level(table, rng):
    """table[k - 1] for the levels of rng, broadcast over i and j"""
    return np.asarray(table, dtype=np.float64)[rng[4] - 1:rng[5]][None, None, :]


def x_curl(m, tables, U, rng):
    """ℑzᵃᵃᶜ(ℑxᶠᵃᵃ w) * ∂z_uˢ at the centre of level k (StokesDrifts.jl:170-171)"""
    W = _Window(m, rng)
    X = lambda dk: _Ix_f(m, W, U["w"], (0, 0, dk))                                 # noqa: E731
    return (X(0) if m.flat[2] else 0.5 * (X(0) + X(1))) * _level(tables[0], rng)


def y_curl(m, tables, U, rng):
    """ℑzᵃᵃᶜ(ℑyᵃᶠᵃ w) * ∂z_vˢ at the centre of level k (:173-174)"""
    W = _Window(m, rng)
    Y = lambda dk: _Iy_f(m, W, U["w"], (0, 0, dk))                                 # noqa: E731
    return (Y(0) if m.flat[2] else 0.5 * (Y(0) + Y(1))) * _level(tables[2], rng)


def z_curl(m, tables, U, rng):
    """(-ℑzᵃᵃᶠ(ℑxᶜᵃᵃ u)) * ∂z_uˢ - ℑzᵃᵃᶠ(ℑyᵃᶜᵃ v) * ∂z_vˢ, both at the face k (:176-178)"""
    W = _Window(m, rng)
    X = lambda dk: _Ix_c(m, W, U["u"], (0, 0, dk))                                 # noqa: E731
    Y = lambda dk: _Iy_c(m, W, U["v"], (0, 0, dk))                                 # noqa: E731
    ua = X(0) if m.flat[2] else 0.5 * (X(-1) + X(0))
    va = Y(0) if m.flat[2] else 0.5 * (Y(-1) + Y(0))
    return (-ua) * _level(tables[1], rng) - va * _level(tables[3], rng)


def add_stokes_drift(m, tables, U, G, rng=None):
    """the three terms in place on G = {"u", "v", "w"} parent arrays that hold everything up to the closure term; each velocity over its
    default range (the wall faces excluded) or over rng"""
    r = _ranges(m, rng)
    if not _empty(r["u"]):
        Gw = _Window(m, r["u"])(G["u"])
        Gw[...] = (Gw + x_curl(m, tables, U, r["u"])) + _level(tables[4], r["u"])
    if not _empty(r["v"]):
        Gw = _Window(m, r["v"])(G["v"])
        Gw[...] = (Gw + y_curl(m, tables, U, r["v"])) + _level(tables[5], r["v"])
    if not _empty(r["w"]):
        Gw = _Window(m, r["w"])(G["w"])
        Gw[...] = (Gw + z_curl(m, tables, U, r["w"])) + 0.0
    return G


class StokesOrchestrated(T.TiltedOrchestrated):
    """TiltedOrchestrated with stokes_drift = the six tables: update_state! adds the terms after the closure term and before the forcing
    (nonhydrostatic_tendency_kernel_functions.jl:99-102)"""

    def __init__(self, O, grid, ntracers, nu, kappa, stokes_tables=None, **kw):
        super().__init__(O, grid, ntracers, nu, kappa, **kw)
        self.stokes_tables = stokes_tables

    def update_state(self, compute_tendencies=True):
        forcing, self.forcing = self.forcing, {}          # the parent's update_state! up to and including the closure term
        try:
            super().update_state(compute_tendencies)
        finally:
            self.forcing = forcing
        if not compute_tendencies:
            return
        if self.stokes_tables is not None:
            add_stokes_drift(self.m, self.stokes_tables, self.U, self.Gn)
        for n, Fa in self.forcing.items():                # G = G_rest + F over the field's cells
            r = self.m.default_range(self.loc[n], n in "uvw")
            Gw = _Window(self.m, r)(self.Gn[n])
            Gw[...] = Gw + np.asarray(Fa)[r[0] - 1:r[1], r[2] - 1:r[3], r[4] - 1:r[5]]
