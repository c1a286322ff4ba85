"""Numpy restatement of flux-form WENO(order = 5) advection with the advecting velocities apart from the advected field (test
infrastructure): the two advection terms of a NonhydrostaticModel with background_fields,

    G_φ = - div(advection, U + Ū, φ) - div(advection, U, Φ̄) + ...     (nonhydrostatic_tendency_kernel_functions.jl:86-94,148-156,213-221,276-293)

every expression with the line of the reference it restates:

  * advective_divergence / advective_tendency -- div_𝐯u, div_𝐯v, div_𝐯w (Advection/momentum_advection_operators.jl:46-83) and div_Uc
                          (tracer_advection_operators.jl:29-33) from the fluxes of upwind_biased_advective_fluxes.jl:23-121
  * BackgroundOrchestrated -- vertically_implicit_reference.Orchestrated whose update_state! forms the total velocities, evaluates both
                          advection terms with the restatement and adds the oracle's pieces for everything else

The oracle has no background fields; with advecting ≡ advected this file is pinned to oro_compute_Gu/Gv/Gw/Gc bit for bit
(tests/test_background_host.py). The nonlinear WENO weights come from the oracle's exported point kernels oro_weno5_biased /
oro_weno3_biased; everything around them -- stencil selection, wall fall-backs, symmetric interpolation of the advecting transport,
upwinding, areas, the divergence -- is restated here. Arrays are PARENT arrays, Fortran order, indexed [i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]."""
import ctypes as C
from fractions import Fraction

import numpy as np

import vertically_implicit_reference as R
from vertically_implicit_reference import BOUNDED, FLAT, LEFT_CONNECTED, LOCS, RIGHT_CONNECTED

# Centered(order = 4) and Centered(order = 2) coefficients as the reference's generated stencils evaluate them in Float64
# (centered_reconstruction.jl, reconstruction_coefficients.jl: the same literals as include/ocn_weno_coeffs.h)
C4 = tuple(float.fromhex(h) for h in ("-0x1.5555555555555p-4", "0x1.2aaaaaaaaaaabp-1", "0x1.2aaaaaaaaaaabp-1", "-0x1.5555555555560p-4"))
C2 = (0.5, 0.5)


def fma(a, b, c):
    """a * b + c with ONE rounding, elementwise (the reference's @muladd compiles to the hardware instruction). Error-free product
    (Dekker) and sums (Knuth): a b + c = r + rr + we exactly with r = fl(s + w); r + fl(rr + we) is the correctly rounded value unless
    rr + we sits within rounding error of a tie (half a spacing of r; a quarter below a power of two) -- those few elements are redone in
    rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    sp = 134217729.0
    ah = a * sp - (a * sp - a)
    al = a - ah
    bh = b * sp - (b * sp - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl           # a b = p + e
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)                               # p + c = s + t
    w = t + e
    wb = w - t
    we = (t - (w - wb)) + (e - wb)                              # t + e = w + we
    r = s + w
    rb = r - s
    rr = (s - (r - rb)) + (w - rb)                              # s + w = r + rr
    q = rr + we
    out = r + q
    ulp = np.spacing(np.abs(r))
    aq = np.abs(q)
    tie = (np.abs(aq - 0.5 * ulp) <= 1e-6 * ulp) | (np.abs(aq - 0.25 * ulp) <= 1e-6 * ulp)
    bad = np.flatnonzero((tie & (we != 0.0)) | ~np.isfinite(out))
    if bad.size:
        out = out.copy()
        af, bf, cf, of = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
        for n in bad:
            if np.isfinite(af[n]) and np.isfinite(bf[n]) and np.isfinite(cf[n]):
                of[n] = float(Fraction(float(af[n])) * Fraction(float(bf[n])) + Fraction(float(cf[n])))
    return out


_POINT = None


def _oracle_lib():
    """the oracle's point kernels through a handle of this module's own (plain addresses as arguments: the loop over points below is the
    cost of the restatement)"""
    global _POINT
    if _POINT is None:
        from oracle import oracle as O
        _POINT = C.CDLL(O.lib()._name)
        for fn in (_POINT.oro_weno5_biased, _POINT.oro_weno3_biased):
            fn.restype, fn.argtypes = C.c_double, [C.c_void_p, C.c_int]
    return _POINT


class _Advection:
    def __init__(self, m):
        self.L, self.m = _oracle_lib(), m
        # adapt_advection_order (adapt_advection_order.jl:62-96): WENO(order = 5) keeps buffer 3 on N >= 3 cells or a Flat direction
        self.B = tuple(3 if (m.topo[d] == FLAT or m.N[d] >= 3) else m.N[d] for d in range(3))
        Hz = m.H[2]
        self.Hz = Hz
        self.ax = m.dy * m.dzc                            # Axᶠᶜᶜ = Δy Δzᶜ (spacings_and_areas_and_volumes.jl:308-335)
        self.ay = m.dx * m.dzc                            # Ayᶜᶠᶜ = Δx Δzᶜ
        self.az = m.dx * m.dy                             # Azᶜᶜᶠ = Δx Δy
        self.vinv_c = 1.0 / ((m.dx * m.dy) * m.dzc)       # V⁻¹ᶜᶜᶜ (:369-378)
        self.vinv_f = 1.0 / ((m.dx * m.dy) * m.dzf)       # V⁻¹ᶜᶜᶠ

    def at(self, a, I, J, K):
        H = self.m.H
        return a[I - 1 + H[0], J - 1 + H[1], K - 1 + H[2]]

    def shift(self, I, J, K, d, n):
        return (I + n, J, K) if d == 0 else ((I, J + n, K) if d == 1 else (I, J, K + n))

    def wall(self, d):
        t = self.m.topo[d]
        return t in (BOUNDED, RIGHT_CONNECTED), t in (BOUNDED, LEFT_CONNECTED)

    # topologically_conditional_interpolation.jl:46-70: `i` is the index the _interpolate function is called with
    def outside_symmetric_halo(self, i, center, N, Rr, lo, hi):
        okl = (i >= Rr if center else i >= Rr + 1) if lo else np.ones_like(i, dtype=bool)
        okh = (i <= N + 1 - Rr) if hi else np.ones_like(i, dtype=bool)
        return okl & okh

    def outside_biased_halo(self, i, center, N, Rr, lo, hi):
        okl = (((i >= Rr) & (i >= Rr - 1)) if center else ((i >= Rr + 1) & (i >= Rr))) if lo else np.ones_like(i, dtype=bool)
        okh = ((i <= N + 1 - (Rr - 1)) & (i <= N + 1 - Rr)) if hi else np.ones_like(i, dtype=bool)
        return okl & okh

    def area_q(self, aq, f, I, J, K):
        """Ax_qᶠᶜᶜ(u), Ay_qᶜᶠᶜ(v), Az_qᶜᶜᶠ(w) (products_between_fields_and_grid_metrics.jl:5-14)"""
        a = self.ax[K - 1 + self.Hz] if aq == 0 else (self.ay[K - 1 + self.Hz] if aq == 1 else self.az)
        return a * self.at(f, I, J, K)

    def symmetric(self, aq, d, center, f, I, J, K, Bflux):
        """_symmetric_interpolate_{x,y,z}ᵃ of the transport along d; Bflux: buffer of the scheme of the direction the flux points along
        (flux_form_advection.jl:45-59). WENO{3}: Centered(order = 4), near a wall Centered(order = 2); reduced schemes: Centered(order = 2)"""
        m = self.m
        if m.topo[d] == FLAT:                             # flat_advective_fluxes.jl:35-50: the identity
            return self.area_q(aq, f, I, J, K)
        o = 1 if center else 0
        q = lambda n: self.area_q(aq, f, *self.shift(I, J, K, d, o - 2 + n))          # noqa: E731
        c2 = lambda: fma(C2[0], q(2), C2[1] * q(1))                                    # noqa: E731
        if Bflux < 3:
            return c2()
        c4 = fma(C4[0], q(3), fma(C4[1], q(2), fma(C4[2], q(1), C4[3] * q(0))))
        lo, hi = self.wall(d)
        if not (lo or hi):
            return c4
        idx = np.broadcast_to((I, J, K)[d], c4.shape)
        return np.where(self.outside_symmetric_halo(idx, center, m.N[d], 3, lo, hi), c4, c2())

    def _weno(self, fn, S, left):
        n = len(S)
        shape = np.broadcast(*S, left).shape
        flat = np.ascontiguousarray(np.stack([np.broadcast_to(s, shape).ravel() for s in S], axis=1))
        lf = np.broadcast_to(left, shape).ravel().astype(np.int32).tolist()
        addr = (flat.ctypes.data + 8 * n * np.arange(flat.shape[0], dtype=np.int64)).tolist()
        return np.array([fn(a, l) for a, l in zip(addr, lf)], dtype=np.float64).reshape(shape)

    def biased(self, d, center, psi, left, I, J, K):
        """_biased_interpolate_{x,y,z}ᵃ of psi along d, left- or right-biased per point: WENO{3}, and within reach of a wall WENO{2}, then
        UpwindBiased{1} (weno_interpolants.jl:504-516 through topologically_conditional_interpolation.jl:46-70)"""
        m, L = self.m, self.L
        o = 1 if center else 0
        s = lambda n: self.at(psi, *self.shift(I, J, K, d, o - 3 + n))                 # noqa: E731   s(n) = psi[idx - 3 + n]
        lo, hi = self.wall(d)
        bounded = lo or hi
        B, N = self.B[d], m.N[d]
        shape = np.broadcast(I, J, K, left).shape
        idx = np.broadcast_to((I, J, K)[d], shape)
        left = np.broadcast_to(left, shape)
        up1 = lambda: np.where(left, 1.0 * np.broadcast_to(s(2), shape), 1.0 * np.broadcast_to(s(3), shape))      # noqa: E731
        if B < 3:
            if B == 2:
                w3 = self._weno(L.oro_weno3_biased, [s(1), s(2), s(3), s(4)], left)
                if not bounded:
                    return w3
                return np.where(self.outside_biased_halo(idx, center, N, 2, lo, hi), w3, up1())
            return up1()
        if not bounded:
            return self._weno(L.oro_weno5_biased, [s(n) for n in range(6)], left)
        in5 = self.outside_biased_halo(idx, center, N, 3, lo, hi)
        in3 = self.outside_biased_halo(idx, center, N, 2, lo, hi)
        out = up1()
        S = [np.broadcast_to(s(n), shape) for n in range(6)]
        if in5.any():
            out[in5] = self._weno(L.oro_weno5_biased, [a[in5] for a in S], left[in5])
        m3 = in3 & ~in5
        if m3.any():
            out[m3] = self._weno(L.oro_weno3_biased, [a[m3] for a in S[1:5]], left[m3])
        return out

    def momentum_flux(self, aq, ds, cs, db, cb, adv, psi, I, J, K):
        """advective_momentum_flux_{U,V,W}{u,v,w} (upwind_biased_advective_fluxes.jl:23-93): the transport `aq` of the advecting velocity
        interpolated along ds, the advected psi reconstructed along db, upwind of the transport's sign"""
        if self.m.topo[db] == FLAT:                       # flat_advective_fluxes.jl:13-27
            return 0.0
        ut = self.symmetric(aq, ds, cs, adv, I, J, K, self.B[db])
        return ut * self.biased(db, cb, psi, ut > 0, I, J, K)

    def tracer_flux(self, d, vel, c, I, J, K):
        """advective_tracer_flux_{x,y,z} (:99-121): A * U[i, j, k] * cᴿ"""
        if self.m.topo[d] == FLAT:
            return 0.0
        ut = self.at(vel, I, J, K)
        cr = self.biased(d, False, c, ut > 0, I, J, K)
        a = self.ax[K - 1 + self.Hz] if d == 0 else (self.ay[K - 1 + self.Hz] if d == 1 else self.az)
        return a * ut * cr


def advective_divergence(m, which, adv, psi, rng=None):
    """div(advection, adv, psi) over the cells of rng (default: the field's cells, periphery excluded for velocities) -> (array over the
    range, range); which: "u" | "v" | "w" | "c"; adv = (ua, va, wa)"""
    A = _Advection(m)
    ua, va, wa = adv
    rng = m.default_range(LOCS[which], which != "c") if rng is None else tuple(rng)
    I = np.arange(rng[0], rng[1] + 1)[:, None, None]
    J = np.arange(rng[2], rng[3] + 1)[None, :, None]
    K = np.arange(rng[4], rng[5] + 1)[None, None, :]
    shape = (I.size, J.size, K.size)
    F = A.momentum_flux
    if which == "u":          # div_𝐯u :46-56: δxᶠᵃᵃ(Uu) + δyᵃᶜᵃ(Vu) + δzᵃᵃᶜ(Wu) at fcc
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = F(0, 0, True, 0, True, ua, psi, I, J, K) - F(0, 0, True, 0, True, ua, psi, I - 1, J, K)
        dy = F(1, 0, False, 1, False, va, psi, I, J + 1, K) - F(1, 0, False, 1, False, va, psi, I, J, K)
        dz = F(2, 0, False, 2, False, wa, psi, I, J, K + 1) - F(2, 0, False, 2, False, wa, psi, I, J, K)
    elif which == "v":        # div_𝐯v :59-69 at cfc
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = F(0, 1, False, 0, False, ua, psi, I + 1, J, K) - F(0, 1, False, 0, False, ua, psi, I, J, K)
        dy = F(1, 1, True, 1, True, va, psi, I, J, K) - F(1, 1, True, 1, True, va, psi, I, J - 1, K)
        dz = F(2, 1, False, 2, False, wa, psi, I, J, K + 1) - F(2, 1, False, 2, False, wa, psi, I, J, K)
    elif which == "w":        # div_𝐯w :72-83 at ccf
        vinv = A.vinv_f[K - 1 + A.Hz]
        dx = F(0, 2, False, 0, False, ua, psi, I + 1, J, K) - F(0, 2, False, 0, False, ua, psi, I, J, K)
        dy = F(1, 2, False, 1, False, va, psi, I, J + 1, K) - F(1, 2, False, 1, False, va, psi, I, J, K)
        dz = F(2, 2, True, 2, True, wa, psi, I, J, K) - F(2, 2, True, 2, True, wa, psi, I, J, K - 1)
    else:                     # div_Uc (tracer_advection_operators.jl:29-33) at ccc
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = A.tracer_flux(0, ua, psi, I + 1, J, K) - A.tracer_flux(0, ua, psi, I, J, K)
        dy = A.tracer_flux(1, va, psi, I, J + 1, K) - A.tracer_flux(1, va, psi, I, J, K)
        dz = A.tracer_flux(2, wa, psi, I, J, K + 1) - A.tracer_flux(2, wa, psi, I, J, K)
    return np.broadcast_to(vinv * ((dx + dy) + dz), shape), rng


def _window(m, a, rng):
    H = m.H
    return a[rng[0] - 1 + H[0]:rng[1] + H[0], rng[2] - 1 + H[1]:rng[3] + H[1], rng[4] - 1 + H[2]:rng[5] + H[2]]


def advective_tendency(m, which, adv, psi, rng=None, G=None, accumulate=False):
    """the advection term of a tendency, written into G (a parent array at the field's location; default: zeros) over rng: G = -div + 0.0
    (`- div - 0 + 0 ...` of the tendency functions, only -0.0 becomes +0.0), or with accumulate G = G - div (the second term of a model
    with background fields). Entries outside rng keep their values."""
    if G is None:
        G = np.zeros(psi.shape, order="F")
    r = m.default_range(LOCS[which], which != "c") if rng is None else tuple(rng)
    if r[1] < r[0] or r[3] < r[2] or r[5] < r[4]:
        return G
    div, r = advective_divergence(m, which, adv, psi, r)
    Gw = _window(m, G, r)
    Gw[...] = (Gw - div) if accumulate else (-div + 0.0)
    return G


class BackgroundOrchestrated(R.Orchestrated):
    """Orchestrated with background_fields = {name: parent array} (names u, v, w, c0, ...; absent: ZeroField), BuoyancyTracer on tracer
    `buoyancy_index`, FPlane(f) and array forcings {name: interior array}. update_state! follows the order of the reference's tendency
    functions: - div(U + Ū, φ) - div(U, Φ̄) - f × U - ∇pHY′ - closure + forcing."""

    def __init__(self, O, grid, ntracers, nu, kappa, background=None, buoyancy_index=None, fcor=None, forcing=None, **kw):
        super().__init__(O, grid, ntracers, nu, kappa, **kw)
        self.bg = {n: (background or {}).get(n) for n in self.names}
        self.b_index, self.fcor, self.forcing = buoyancy_index, fcor, dict(forcing or {})
        self.pHY = grid.zeros(LOCS["c"]) if buoyancy_index is not None else None
        self.total = None

    def total_velocities(self):
        """SumOfArrays{2} (Utils/sum_of_arrays.jl:23,39-41): one addition per access; a ZeroField background leaves the model's array"""
        return tuple(self.U[n] if self.bg[n] is None else self.U[n] + self.bg[n] for n in "uvw")

    def update_state(self, compute_tendencies=True):
        g, U, L, O = self.g, self.U, self.L, self.O
        for n in self.names:
            self._fill(n, False)
        if self.b_index is not None:                      # compute_auxiliaries!: update_hydrostatic_pressure! with the model's b only
            L.oro_update_hydrostatic_pressure(g.handle, 1, O._dp(U["c%d" % self.b_index]), None, 0.0, 0.0, 0.0, O._dp(self.pHY))
        self.total = self.total_velocities()
        if not compute_tendencies:
            return
        own = (U["u"], U["v"], U["w"])
        for n in self.names:
            which = n if n in "uvw" else "c"
            advective_tendency(self.m, which, self.total, U[n], G=self.Gn[n])
            if self.bg[n] is not None:                    # div(…, U, ::ZeroField) = 0: no second term without a background
                advective_tendency(self.m, which, own, self.bg[n], G=self.Gn[n], accumulate=True)
        if self.fcor is not None:
            L.oro_add_fplane_coriolis(g.handle, float(self.fcor), O._dp(U["u"]), O._dp(U["v"]), O._dp(self.Gn["u"]), O._dp(self.Gn["v"]))
        if self.b_index is not None:
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
            Gw = _window(self.m, self.Gn[n], r)
            Gw[...] = Gw + np.asarray(Fa)[r[0] - 1:r[1], r[2] - 1:r[3], r[4] - 1:r[5]]
