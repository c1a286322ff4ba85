"""Numpy restatement of the terms of a tilted domain (test infrastructure), every expression with the line of the reference it restates:

  * x_f_cross_U / y_f_cross_U / z_f_cross_U -- ConstantCartesianCoriolis (Coriolis/constant_cartesian_coriolis.jl:70-81)
  * x_dot_g_b / y_dot_g_b                   -- BuoyancyForce(formulation; gravity_unit_vector) (BuoyancyFormulations/g_dot_b.jl:2-3,
                                               buoyancy_force.jl:52-54)
  * hydrostatic_pressure                    -- _update_hydrostatic_pressure! with z_dot_g_b = ĝ_z ℑzᵃᵃᶠ(b) (update_hydrostatic_pressure.jl:12-22,
                                               g_dot_b.jl:4)
  * TiltedOrchestrated                      -- background_reference.BackgroundOrchestrated whose update_state! inserts these terms in the order
                                               of the reference's tendency functions (nonhydrostatic_tendency_kernel_functions.jl:93-102,
                                               155-164,220-228)

The oracle has neither; tests/test_tilted_host.py pins this file to it where they overlap (ĝ = ẑ against oro_update_hydrostatic_pressure, f =
(0, 0, f) against oro_add_fplane_coriolis) and to the analytic f × U where every product is exact. Every operation is an elementwise IEEE
float64 operation in the stated association order. Arrays are PARENT arrays, Fortran order, indexed [i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]."""
import numpy as np

import background_reference as B
import vertically_implicit_reference as R
from vertically_implicit_reference import LOCS, _Window


# ---------------------------------------------------------------------------------------------------------------------
# interpolations (Operators/interpolation_operators.jl:10-38); along a Flat direction the identity (:87-112). `f(di, dj, dk)` is the
# interpolated function at (i + di, j + dj, k + dk) over the window
# ---------------------------------------------------------------------------------------------------------------------
def _Ix_c(m, W, a, o):       # ℑxᶜᵃᵃ: (a[i] + a[i + 1]) / 2
    return W(a, *o) if m.flat[0] else 0.5 * (W(a, *o) + W(a, o[0] + 1, o[1], o[2]))


def _Iy_c(m, W, a, o):       # ℑyᵃᶜᵃ: (a[j] + a[j + 1]) / 2
    return W(a, *o) if m.flat[1] else 0.5 * (W(a, *o) + W(a, o[0], o[1] + 1, o[2]))


def _Iz_c(m, W, a, o):       # ℑzᵃᵃᶜ: (a[k] + a[k + 1]) / 2
    return W(a, *o) if m.flat[2] else 0.5 * (W(a, *o) + W(a, o[0], o[1], o[2] + 1))


def x_f_cross_U(m, f, U, rng):
    """ℑxᶠᵃᵃ(fʸw_minus_fᶻv) (:70-71,79) over the cells of rng; f = (fx, fy, fz), U = {"u", "v", "w"} parent arrays"""
    W = _Window(m, rng)
    A = lambda di: f[1] * _Iz_c(m, W, U["w"], (di, 0, 0)) - f[2] * _Iy_c(m, W, U["v"], (di, 0, 0))       # noqa: E731
    return A(0) if m.flat[0] else 0.5 * (A(-1) + A(0))


def y_f_cross_U(m, f, U, rng):
    """ℑyᵃᶠᵃ(fᶻu_minus_fˣw) (:73-74,80)"""
    W = _Window(m, rng)
    Bf = lambda dj: f[2] * _Ix_c(m, W, U["u"], (0, dj, 0)) - f[0] * _Iz_c(m, W, U["w"], (0, dj, 0))      # noqa: E731
    return Bf(0) if m.flat[1] else 0.5 * (Bf(-1) + Bf(0))


def z_f_cross_U(m, f, U, rng):
    """ℑzᵃᵃᶠ(fˣv_minus_fʸu) (:76-77,81)"""
    W = _Window(m, rng)
    Cf = lambda dk: f[0] * _Iy_c(m, W, U["v"], (0, 0, dk)) - f[1] * _Ix_c(m, W, U["u"], (0, 0, dk))      # noqa: E731
    return Cf(0) if m.flat[2] else 0.5 * (Cf(-1) + Cf(0))


def buoyancy_perturbation(kind, bT, S=None, g=0.0, alpha=0.0, beta=0.0):
    """buoyancy_perturbationᶜᶜᶜ over the parent array: the tracer (buoyancy_tracer.jl:12), or g (α T - β S)
    (seawater_buoyancy.jl, linear_equation_of_state.jl:71-73)"""
    return bT if kind == 1 else g * (alpha * bT - beta * S)


def x_dot_g_b(m, ghat_x, b, rng):
    """x_dot_g_bᶠᶜᶜ = ĝ_x * ℑxᶠᵃᵃ(b) (g_dot_b.jl:2); b: the buoyancy perturbation, a ccc parent array"""
    W = _Window(m, rng)
    return ghat_x * (W(b) if m.flat[0] else 0.5 * (W(b, -1, 0, 0) + W(b)))


def y_dot_g_b(m, ghat_y, b, rng):
    """y_dot_g_bᶜᶠᶜ = ĝ_y * ℑyᵃᶠᵃ(b) (g_dot_b.jl:3)"""
    W = _Window(m, rng)
    return ghat_y * (W(b) if m.flat[1] else 0.5 * (W(b, 0, -1, 0) + W(b)))


def hydrostatic_pressure(m, ghat_z, b, pHY):
    """_update_hydrostatic_pressure! (update_hydrostatic_pressure.jl:12-22) over i = 0:Nx+1, j = 0:Ny+1 (:43-50; a Flat direction: its one
    cell), in place: pHY′[Nz] = - z_dot_g_b(Nz+1) Δzᶠ(Nz+1); pHY′[k] = pHY′[k+1] - z_dot_g_b(k+1) Δzᶠ(k+1) with z_dot_g_bᶜᶜᶠ = ĝ_z *
    ℑzᵃᵃᶠ(b) (g_dot_b.jl:4). A Flat z: nothing (update_hydrostatic_pressure!(::ZFlatGrid))"""
    if m.flat[2]:
        return pHY
    Nx, Ny, Nz = m.N
    Hx, Hy, Hz = m.H
    si = slice(Hx, Hx + 1) if m.flat[0] else slice(Hx - 1, Hx + Nx + 1)
    sj = slice(Hy, Hy + 1) if m.flat[1] else slice(Hy - 1, Hy + Ny + 1)
    at = lambda a, k: a[si, sj, k - 1 + Hz]                                     # noqa: E731
    zb = lambda kf: ghat_z * (0.5 * (at(b, kf - 1) + at(b, kf)))                # noqa: E731   at the face kf
    p = -zb(Nz + 1) * m.dzf[Nz + Hz]
    pHY[si, sj, Nz - 1 + Hz] = p
    for k in range(Nz - 1, 0, -1):
        p = p - zb(k + 1) * m.dzf[k + Hz]
        pHY[si, sj, k - 1 + Hz] = p
    return pHY


def _ranges(m, rng):
    """the range of each velocity: its default (the wall faces excluded) or the given one"""
    return {n: (m.default_range(LOCS[n], True) if rng is None else tuple(rng)) for n in "uvw"}


def _empty(r):
    return r[1] < r[0] or r[3] < r[2] or r[5] < r[4]


def add_cartesian_coriolis(m, f, U, G, rng=None):
    """G_u -= x_f_cross_U, G_v -= y_f_cross_U, G_w -= z_f_cross_U (nonhydrostatic_tendency_kernel_functions.jl:96,158,223) in place; G =
    {"u", "v", "w"} parent arrays holding the advective part"""
    term = {"u": x_f_cross_U, "v": y_f_cross_U, "w": z_f_cross_U}
    for n, r in _ranges(m, rng).items():
        if not _empty(r):
            Gw = _Window(m, r)(G[n])
            Gw[...] = Gw - term[n](m, f, U, r)
    return G


def add_buoyancy_acceleration(m, ghat, b, G, rng=None):
    """G_u += x_dot_g_b, G_v += y_dot_g_b (nonhydrostatic_tendency_kernel_functions.jl:95,157) in place"""
    r = _ranges(m, rng)
    if not _empty(r["u"]):
        Gw = _Window(m, r["u"])(G["u"])
        Gw[...] = Gw + x_dot_g_b(m, ghat[0], b, r["u"])
    if not _empty(r["v"]):
        Gw = _Window(m, r["v"])(G["v"])
        Gw[...] = Gw + y_dot_g_b(m, ghat[1], b, r["v"])
    return G


class TiltedOrchestrated(B.BackgroundOrchestrated):
    """BackgroundOrchestrated with coriolis = ConstantCartesianCoriolis(*cartesian) and buoyancy = BuoyancyForce(BuoyancyTracer();
    gravity_unit_vector) on tracer `buoyancy_index`. update_state! in the order of the reference's tendency functions:
    - div(U + Ū, φ) - div(U, Φ̄) + x/y_dot_g_b - f × U - ∇pHY′ - closure + forcing; w: - div ... - z_f_cross_U - closure."""

    def __init__(self, O, grid, ntracers, nu, kappa, cartesian=None, gravity_unit_vector=None, **kw):
        super().__init__(O, grid, ntracers, nu, kappa, **kw)
        self.cartesian = None if cartesian is None else tuple(float(c) for c in cartesian)
        # ĝ = -gravity_unit_vector (buoyancy_force.jl:52-54); None: NegativeZDirection(), ĝ = (0, 0, 1) and no x / y terms
        self.ghat = None if gravity_unit_vector is None else tuple(-float(c) for c in gravity_unit_vector)
        assert self.fcor is None or self.cartesian is None, "the model has one Coriolis"
        assert self.ghat is None or self.b_index is not None

    def update_state(self, compute_tendencies=True):
        g, U, L, O = self.g, self.U, self.L, self.O
        for n in self.names:
            self._fill(n, False)
        b = U["c%d" % self.b_index] if self.b_index is not None else None
        if b is not None:                                 # compute_auxiliaries!: update_hydrostatic_pressure!
            if self.ghat is None:
                L.oro_update_hydrostatic_pressure(g.handle, 1, O._dp(b), None, 0.0, 0.0, 0.0, O._dp(self.pHY))
            else:
                hydrostatic_pressure(self.m, self.ghat[2], b, self.pHY)
        self.total = self.total_velocities()
        if not compute_tendencies:
            return
        own = (U["u"], U["v"], U["w"])
        any_bg = any(self.bg[n] is not None for n in self.names)
        for n in self.names:
            which = n if n in "uvw" else "c"
            if not any_bg:                                # the oracle's advection: what the restatement is pinned to (test_background_host.py)
                g.compute_G(which, U["u"], U["v"], U["w"], self.Gn[n], c=None if n in "uvw" else U[n])
                continue
            B.advective_tendency(self.m, which, self.total, U[n], G=self.Gn[n])
            if self.bg[n] is not None:
                B.advective_tendency(self.m, which, own, self.bg[n], G=self.Gn[n], accumulate=True)
        if self.ghat is not None:
            add_buoyancy_acceleration(self.m, self.ghat, b, self.Gn)
        if self.cartesian is not None:
            add_cartesian_coriolis(self.m, self.cartesian, U, self.Gn)
        if self.fcor is not None:
            L.oro_add_fplane_coriolis(g.handle, float(self.fcor), O._dp(U["u"]), O._dp(U["v"]), O._dp(self.Gn["u"]), O._dp(self.Gn["v"]))
        if b is not None:
            L.oro_add_hydrostatic_pressure_gradient(g.handle, O._dp(self.pHY), O._dp(self.Gn["u"]), O._dp(self.Gn["v"]))
        if self.nu != 0.0 or any(self.kappa):
            for f, n in enumerate(self.names):
                which = n if n in "uvw" else "c"
                if self.closure == "oracle":
                    c = U[n] if which == "c" else None
                    L.oro_add_closure_tendency(g.handle, min(f, 3), O._dp(U["u"]), O._dp(U["v"]), O._dp(U["w"]), O._dp(c) if c is not None else None,
                                               self.coef(n), O._dp(self.Gn[n]), None)
                else:
                    R.explicit_part(self.m, which, U, U[n], self.coef(n), self.Gn[n], vi=self.closure == "vi")
        for n, Fa in self.forcing.items():                # G = G_rest + F over the field's cells
            r = self.m.default_range(self.loc[n], n in "uvw")
            Gw = B._window(self.m, self.Gn[n], r)
            Gw[...] = Gw + np.asarray(Fa)[r[0] - 1:r[1], r[2] - 1:r[3], r[4] - 1:r[5]]
