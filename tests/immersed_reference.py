"""Numpy restatement of a NonhydrostaticModel on an ImmersedBoundaryGrid with a grid-fitted boundary (test infrastructure), every
expression with the line of the reference it restates:

  * immersed_cells          -- materialize_immersed_boundary + _immersed_cell of GridFittedBottom (grid_fitted_bottom.jl:99-130, the snapping
                               loop :111-122) and GridFittedBoundary (grid_fitted_boundary.jl:14-32), halos filled with the default conditions
  * Immersed                -- inactive_cell / inactive_node / peripheral_node / immersed_peripheral_node at all eight locations
                               (Grids/inactive_node.jl:43-162, immersed_boundary_interface.jl:49-54) and the two flag tables of
                               csrc/ocn_immersed.h (the windows of inside_immersed_boundary, immersed_advective_fluxes.jl:121-152)
  * ImmersedAdvection       -- background_reference._Advection whose cascade reads the immersed windows (:154-220) and whose fluxes are
                               conditional_flux_* (:20-59)
  * immersed_closure_part   -- the explicit ScalarDiffusivity term with every flux conditional (immersed_diffusive_fluxes.jl:27-44)
  * fplane                  -- x_f_cross_U / y_f_cross_U with the active-weighted average (Coriolis/f_plane.jl:48-52,
                               Operators/interpolation_operators.jl:116-130) whose not_peripheral counts the immersed cells
  * ImmersedOrchestrated    -- vertically_implicit_reference.Orchestrated with the two masks (update_nonhydrostatic_model_state.jl:22-25,
                               pressure_correction.jl:10-12), the masked set! (set_nonhydrostatic_model.jl:47-49), BuoyancyTracer, FPlane
                               and array forcings

A shift along a Flat direction is no shift (one cell, no halo: its Face is its Center). Arrays are PARENT arrays, Fortran order, indexed
[i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]; with no immersed cell everything here equals background_reference / the oracle bit for bit
(tests/test_immersed_host.py)."""
import numpy as np

import background_reference as B
import vertically_implicit_reference as R
from vertically_implicit_reference import BOUNDED, CENTER, FACE, FLAT, LEFT_CONNECTED, LOCS, PERIODIC, RIGHT_CONNECTED

# bit of the periphery byte per location (csrc/ocn_immersed.h): inactive_cell, then immersed_peripheral_node at fcc .. ccc
BIT = {"inactive": 0, (FACE, CENTER, CENTER): 1, (CENTER, FACE, CENTER): 2, (CENTER, CENTER, FACE): 3, (FACE, FACE, CENTER): 4,
       (FACE, CENTER, FACE): 5, (CENTER, FACE, FACE): 6, (CENTER, CENTER, CENTER): 7}
ALL_LOCATIONS = [(a, b, c) for a in (CENTER, FACE) for b in (CENTER, FACE) for c in (CENTER, FACE)]


# ---------------------------------------------------------------------------------------------------------------------
# the boundary -> immersed_cell over the parent extent
# ---------------------------------------------------------------------------------------------------------------------
def fill_center_halo(a, d, N, H, topo):
    """fill_halo_regions! of a Center field along d with its default condition: Periodic copies node N + 1 - h to 1 - h and node h to
    N + h; next to a wall the no-flux mirror copies node h to 1 - h and node N + 1 - h to N + h"""
    ix = lambda node: tuple(node - 1 + H if q == d else slice(None) for q in range(a.ndim))          # noqa: E731
    for h in range(1, H + 1):
        if topo == PERIODIC:
            a[ix(1 - h)], a[ix(N + h)] = a[ix(N + 1 - h)], a[ix(h)]
        else:
            a[ix(1 - h)], a[ix(N + h)] = a[ix(h)], a[ix(N + 1 - h)]


def immersed_cells(m, zf, zc, xc=None, yc=None, bottom=None, interface=False, mask=None):
    """-> (immersed_cell over the parent extent, the numerical bottom height over its parent extent or None).
    zf, zc: the z face / centre nodes WITH halos (array position Hz holds node 1); xc, yc: interior centre nodes.
    bottom: a number, an (Nx, Ny) array or f(non-Flat horizontal coordinates); mask: an (Nx, Ny, Nz) array or f(non-Flat coordinates)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = m.N, m.H
    P = (Nx + 2 * Hx, Ny + 2 * Hy, Nz + 2 * Hz)
    if bottom is not None:
        if callable(bottom):
            zb = np.empty((Nx, Ny))
            for i in range(Nx):
                for j in range(Ny):
                    pair = (xc[i] if xc is not None else None, yc[j] if yc is not None else None)
                    zb[i, j] = bottom(*[c for c, t in zip(pair, m.topo[:2]) if t != FLAT])
        else:
            zb = np.full((Nx, Ny), float(bottom)) if np.ndim(bottom) == 0 else np.asarray(bottom, dtype=np.float64).reshape(Nx, Ny)
        num = np.empty(P[:2])
        for i in range(Nx):
            for j in range(Ny):
                v = zf[Hz]                                            # rnode(i, j, 1, grid, c, c, f)
                for k in range(1, Nz + 1):                            # grid_fitted_bottom.jl:116-121
                    zp, z = zf[k + Hz], zc[k - 1 + Hz]
                    if (zp <= zb[i, j]) if interface else (z <= zb[i, j]):
                        v = zp
                num[i + Hx, j + Hy] = v
        for d in (0, 1):
            if m.topo[d] != FLAT:
                fill_center_halo(num, d, m.N[d], m.H[d], m.topo[d])
        cell = np.zeros(P, dtype=bool, order="F")
        for k in range(P[2]):
            cell[:, :, k] = zc[k] <= num                              # _immersed_cell: z <= zb at every level, halos included
        return cell, num
    vals = np.zeros(m.N, dtype=bool)
    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz):
                if callable(mask):
                    c3 = (xc[i] if xc is not None else None, yc[j] if yc is not None else None, zc[k + Hz])
                    vals[i, j, k] = bool(mask(*[c for c, t in zip(c3, m.topo) if t != FLAT]))
                else:
                    vals[i, j, k] = bool(np.asarray(mask).reshape(m.N)[i, j, k])
    cell = np.zeros(P, dtype=bool, order="F")
    cell[Hx:Hx + Nx, Hy:Hy + Ny, Hz:Hz + Nz] = vals
    for d in range(3):
        if m.topo[d] != FLAT:
            fill_center_halo(cell, d, m.N[d], m.H[d], m.topo[d])
    return cell, None


def cells_of_grid(grid, boundary, m=None):
    """immersed_cells for a RectilinearGrid of the package and a boundary description dict(bottom=..., interface=...) | dict(mask=...)"""
    m = R.Metrics.of_grid(grid) if m is None else m
    H = grid.halo_size
    xc = None if m.topo[0] == FLAT else np.asarray(grid.xᶜᵃᵃ)[H[0]:H[0] + grid.Nx]
    yc = None if m.topo[1] == FLAT else np.asarray(grid.yᵃᶜᵃ)[H[1]:H[1] + grid.Ny]
    return immersed_cells(m, np.asarray(grid.zᵃᵃᶠ), np.asarray(grid.zᵃᵃᶜ), xc, yc, **boundary)


# ---------------------------------------------------------------------------------------------------------------------
# predicates and flag tables
# ---------------------------------------------------------------------------------------------------------------------
class Immersed:
    def __init__(self, m, cell):
        self.m, self.cell = m, np.asarray(cell, dtype=bool)
        assert self.cell.shape == tuple(n + 2 * h for n, h in zip(m.N, m.H))
        self.periphery, self.orders = self.flag_tables()

    # ---- cells ----
    def immersed_cell(self, I, J, K):
        """the mask entry; False beyond the parent extent (no entry there: only a direction without a wall gets there, see ocn_immersed.h).
        A Flat direction ignores its index."""
        idx, ok = [], True
        for d, x in enumerate((I, J, K)):
            if self.m.topo[d] == FLAT:
                idx.append(np.zeros_like(np.asarray(x)))
                continue
            p = np.asarray(x) - 1 + self.m.H[d]
            ok = ok & (p >= 0) & (p < self.cell.shape[d])
            idx.append(np.clip(p, 0, self.cell.shape[d] - 1))
        return self.cell[tuple(np.broadcast_arrays(*idx))] & ok

    def inactive_cell(self, I, J, K, underlying=False):
        """immersed_boundary_interface.jl:49: immersed_cell | inactive_cell(underlying grid)"""
        out = R._inactive_cell(self.m, I, J, K)
        return out if underlying else (out | self.immersed_cell(I, J, K))

    def _down(self, I, J, K, d):
        if self.m.topo[d] == FLAT:
            return I, J, K
        return (I - 1, J, K) if d == 0 else ((I, J - 1, K) if d == 1 else (I, J, K - 1))

    def node(self, I, J, K, loc, peripheral, underlying=False):
        """inactive_node (inactive_node.jl:127-137: `&` over the cells around the node) / peripheral_node (:152-162: `|`)"""
        op = np.logical_or if peripheral else np.logical_and
        for d in range(3):
            if loc[d] == FACE:
                rest = tuple(CENTER if q == d else l for q, l in enumerate(loc))
                return op(self.node(I, J, K, rest, peripheral, underlying), self.node(*self._down(I, J, K, d), rest, peripheral, underlying))
        return self.inactive_cell(I, J, K, underlying)

    def inactive_node(self, I, J, K, loc, underlying=False):
        return self.node(I, J, K, loc, False, underlying)

    def peripheral_node(self, I, J, K, loc, underlying=False):
        return self.node(I, J, K, loc, True, underlying)

    def immersed_peripheral_node(self, I, J, K, loc):
        """immersed_boundary_interface.jl:53-54"""
        return self.peripheral_node(I, J, K, loc) & ~self.peripheral_node(I, J, K, loc, underlying=True)

    # ---- the tables ----
    def parent_indices(self):
        return tuple(np.arange(1 - h, n + h + 1).reshape([-1 if q == d else 1 for q in range(3)]) for d, (n, h) in enumerate(zip(self.m.N, self.m.H)))

    def window_free(self, I, J, K, d, center, b):
        """no inactive node in the window of buffer b along d on side ᶠ (center False) / ᶜ (immersed_advective_fluxes.jl:121-152): offsets
        -b .. b - 1 at (c, c, c), or 1 - b .. b at the Face along d"""
        loc = tuple(FACE if (center and q == d) else CENTER for q in range(3))
        near = False
        for c in (range(1 - b, b + 1) if center else range(-b, b)):
            at = [I, J, K]
            at[d] = at[d] + c
            near = near | self.inactive_node(*at, loc)
        return ~near

    def flag_tables(self):
        I, J, K = self.parent_indices()
        shape = self.cell.shape
        periphery = np.broadcast_to(self.inactive_cell(I, J, K), shape).astype(np.uint8)
        for loc, bit in BIT.items():
            if loc != "inactive":
                periphery = periphery | (np.broadcast_to(self.immersed_peripheral_node(I, J, K, loc), shape).astype(np.uint8) << bit)
        orders = np.zeros(shape, dtype=np.uint16)
        for d in range(3):
            for side in (0, 1):
                if self.m.topo[d] == FLAT:
                    best = np.full(shape, 3, dtype=np.uint16)
                else:
                    best = np.ones(shape, dtype=np.uint16)
                    for b in (2, 3):
                        best = np.where(np.broadcast_to(self.window_free(I, J, K, d, bool(side), b), shape), np.uint16(b), best)
                orders = orders | (best << np.uint16(2 * (2 * d + side)))
        return np.asfortranarray(periphery), np.asfortranarray(orders)

    def _lookup(self, table, I, J, K):
        idx = [np.zeros_like(np.asarray(x)) if self.m.topo[d] == FLAT else np.asarray(x) - 1 + self.m.H[d] for d, x in enumerate((I, J, K))]
        for d, p in enumerate(idx):
            assert p.min() >= 0 and p.max() < table.shape[d], "a flag is read beyond the parent extent"
        return table[tuple(np.broadcast_arrays(*idx))]

    def bit(self, loc, I, J, K):
        return ((self._lookup(self.periphery, I, J, K) >> BIT[loc]) & 1).astype(bool)

    def order(self, d, center, I, J, K):
        return (self._lookup(self.orders, I, J, K) >> (2 * (2 * d + int(center)))) & 3

    def mask_field(self, a, loc, value=0.0):
        """mask_immersed_field! (mask_immersed_field.jl:53-64) over :xyz, in place on a parent array"""
        I, J, K = (np.arange(1, n + 1).reshape([-1 if q == d else 1 for q in range(3)]) for d, n in enumerate(self.m.N))
        masked = np.broadcast_to(self.bit(tuple(loc), I, J, K), self.m.N)
        Hx, Hy, Hz = self.m.H
        view = a[Hx:Hx + self.m.N[0], Hy:Hy + self.m.N[1], Hz:Hz + self.m.N[2]]
        view[masked] = value
        return a


# ---------------------------------------------------------------------------------------------------------------------
# advection
# ---------------------------------------------------------------------------------------------------------------------
def _flux_location(ds, db):
    """where advective_momentum_flux of a Face-along-ds field along db lives (immersed_advective_fluxes.jl:39-55)"""
    return tuple(FACE if (ds != db and q in (ds, db)) else CENTER for q in range(3))


class ImmersedAdvection(B._Advection):
    def __init__(self, m, imm):
        super().__init__(m)
        self.imm = imm

    def symmetric(self, aq, d, center, f, I, J, K, Bflux):
        m = self.m
        if m.topo[d] == FLAT:
            return self.area_q(aq, f, I, J, K)
        o = 1 if center else 0
        q = lambda n: self.area_q(aq, f, *self.shift(I, J, K, d, o - 2 + n))          # noqa: E731
        c2 = B.fma(B.C2[0], q(2), B.C2[1] * q(1))
        if Bflux < 3:
            return c2
        c4 = B.fma(B.C4[0], q(3), B.fma(B.C4[1], q(2), B.fma(B.C4[2], q(1), B.C4[3] * q(0))))
        order = np.broadcast_to(self.imm.order(d, center, I, J, K), np.broadcast(c4, I, J, K).shape)
        return np.where(order >= 3, c4, c2)

    def biased(self, d, center, psi, left, I, J, K):
        L = self.L
        o = 1 if center else 0
        s = lambda n: self.at(psi, *self.shift(I, J, K, d, o - 3 + n))                 # noqa: E731
        shape = np.broadcast(I, J, K, left).shape
        left = np.broadcast_to(left, shape)
        order = np.minimum(self.B[d], np.broadcast_to(self.imm.order(d, center, I, J, K), shape))
        out = np.where(left, 1.0 * np.broadcast_to(s(2), shape), 1.0 * np.broadcast_to(s(3), shape))
        in5, in3 = order >= 3, order == 2
        if in5.any():
            S = [np.broadcast_to(s(n), shape) for n in range(6)]
            out[in5] = self._weno(L.oro_weno5_biased, [a[in5] for a in S], left[in5])
        if in3.any():
            S = [np.broadcast_to(s(n), shape) for n in range(1, 5)]
            out[in3] = self._weno(L.oro_weno3_biased, [a[in3] for a in S], left[in3])
        return out

    def momentum_flux(self, aq, ds, cs, db, cb, adv, psi, I, J, K):
        if self.m.topo[db] == FLAT:
            return 0.0
        flux = super().momentum_flux(aq, ds, cs, db, cb, adv, psi, I, J, K)
        return np.where(self.imm.bit(_flux_location(ds, db), I, J, K), 0.0, flux)

    def tracer_flux(self, d, vel, c, I, J, K):
        if self.m.topo[d] == FLAT:
            return 0.0
        flux = super().tracer_flux(d, vel, c, I, J, K)
        return np.where(self.imm.bit(tuple(FACE if q == d else CENTER for q in range(3)), I, J, K), 0.0, flux)


def advective_tendency(m, imm, which, adv, psi, rng=None, G=None, accumulate=False):
    """background_reference.advective_tendency on an immersed grid: the same divergences (momentum_advection_operators.jl:46-83,
    tracer_advection_operators.jl:29-33) of ImmersedAdvection's fluxes"""
    A = ImmersedAdvection(m, imm)
    ua, va, wa = adv
    if G is None:
        G = np.zeros(psi.shape, order="F")
    r = m.default_range(LOCS[which], which != "c") if rng is None else tuple(rng)
    if r[1] < r[0] or r[3] < r[2] or r[5] < r[4]:
        return G
    I = np.arange(r[0], r[1] + 1)[:, None, None]
    J = np.arange(r[2], r[3] + 1)[None, :, None]
    K = np.arange(r[4], r[5] + 1)[None, None, :]
    F = A.momentum_flux
    if which == "u":
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = F(0, 0, True, 0, True, ua, psi, I, J, K) - F(0, 0, True, 0, True, ua, psi, I - 1, J, K)
        dy = F(1, 0, False, 1, False, va, psi, I, J + 1, K) - F(1, 0, False, 1, False, va, psi, I, J, K)
        dz = F(2, 0, False, 2, False, wa, psi, I, J, K + 1) - F(2, 0, False, 2, False, wa, psi, I, J, K)
    elif which == "v":
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = F(0, 1, False, 0, False, ua, psi, I + 1, J, K) - F(0, 1, False, 0, False, ua, psi, I, J, K)
        dy = F(1, 1, True, 1, True, va, psi, I, J, K) - F(1, 1, True, 1, True, va, psi, I, J - 1, K)
        dz = F(2, 1, False, 2, False, wa, psi, I, J, K + 1) - F(2, 1, False, 2, False, wa, psi, I, J, K)
    elif which == "w":
        vinv = A.vinv_f[K - 1 + A.Hz]
        dx = F(0, 2, False, 0, False, ua, psi, I + 1, J, K) - F(0, 2, False, 0, False, ua, psi, I, J, K)
        dy = F(1, 2, False, 1, False, va, psi, I, J + 1, K) - F(1, 2, False, 1, False, va, psi, I, J, K)
        dz = F(2, 2, True, 2, True, wa, psi, I, J, K) - F(2, 2, True, 2, True, wa, psi, I, J, K - 1)
    else:
        vinv = A.vinv_c[K - 1 + A.Hz]
        dx = A.tracer_flux(0, ua, psi, I + 1, J, K) - A.tracer_flux(0, ua, psi, I, J, K)
        dy = A.tracer_flux(1, va, psi, I, J + 1, K) - A.tracer_flux(1, va, psi, I, J, K)
        dz = A.tracer_flux(2, wa, psi, I, J, K + 1) - A.tracer_flux(2, wa, psi, I, J, K)
    div = np.broadcast_to(vinv * ((dx + dy) + dz), (I.size, J.size, K.size))
    Gw = B._window(m, G, r)
    Gw[...] = (Gw - div) if accumulate else (-div + 0.0)
    return G


# ---------------------------------------------------------------------------------------------------------------------
# the explicit closure term, every flux conditional
# ---------------------------------------------------------------------------------------------------------------------
def immersed_closure_part(m, imm, which, P, c, coef, G, rng=None):
    """G = (G - ∂ⱼτᵢⱼ | ∇·q) + 0 with _viscous_flux_* / _diffusive_flux_* of immersed_diffusive_fluxes.jl:27-44: the fluxes of
    vertically_implicit_reference.closure_divergence (explicit), each zero where its own location is an immersed_peripheral_node"""
    if coef == 0.0:
        return G
    rng = m.default_range(LOCS[which], which != "c") if rng is None else tuple(rng)
    if rng[1] < rng[0] or rng[3] < rng[2] or rng[5] < rng[4]:
        return G
    W = R._Window(m, rng)
    u, v, w = P["u"], P["v"], P["w"]
    fx, fy, fz = m.flat
    I = np.arange(rng[0], rng[1] + 1)[:, None, None]
    J = np.arange(rng[2], rng[3] + 1)[None, :, None]
    K = np.arange(rng[4], rng[5] + 1)[None, None, :]
    shape = (I.size, J.size, K.size)

    def cond(loc, o, flux):
        return np.where(np.broadcast_to(imm.bit(loc, I + o[0], J + o[1], K + o[2]), shape), 0.0, flux)

    ccc, ffc, fcf, cff = (CENTER,) * 3, (FACE, FACE, CENTER), (FACE, CENTER, FACE), (CENTER, FACE, FACE)
    vf = lambda s: -(2 * (coef * s))                                                        # noqa: E731
    f11 = lambda o: cond(ccc, o, vf(W.ddx_c(u, o)))                                         # noqa: E731
    f22 = lambda o: cond(ccc, o, vf(W.ddy_c(v, o)))                                         # noqa: E731
    f33 = lambda o: cond(ccc, o, vf(W.ddz_c(w, o)))                                         # noqa: E731
    f12 = lambda o: cond(ffc, o, vf(0.5 * (W.ddy_f(u, o) + W.ddx_f(v, o))))                 # noqa: E731
    f13 = lambda o: cond(fcf, o, vf(0.5 * (W.ddz_f(u, o) + W.ddx_f(w, o))))                 # noqa: E731
    f23 = lambda o: cond(cff, o, vf(0.5 * (W.ddz_f(v, o) + W.ddy_f(w, o))))                 # noqa: E731
    dx_, dy_ = m.dx, m.dy
    az = dx_ * dy_
    if which == "u":
        dz_ = W.level(m.dzc)
        dx = 0.0 if fx else (dy_ * dz_) * f11((0, 0, 0)) - (dy_ * dz_) * f11((-1, 0, 0))
        dy = 0.0 if fy else (dx_ * dz_) * f12((0, 1, 0)) - (dx_ * dz_) * f12((0, 0, 0))
        dz = 0.0 if fz else az * f13((0, 0, 1)) - az * f13((0, 0, 0))
    elif which == "v":
        dz_ = W.level(m.dzc)
        dx = 0.0 if fx else (dy_ * dz_) * f12((1, 0, 0)) - (dy_ * dz_) * f12((0, 0, 0))
        dy = 0.0 if fy else (dx_ * dz_) * f22((0, 0, 0)) - (dx_ * dz_) * f22((0, -1, 0))
        dz = 0.0 if fz else az * f23((0, 0, 1)) - az * f23((0, 0, 0))
    elif which == "w":
        dz_ = W.level(m.dzf)
        dx = 0.0 if fx else (dy_ * dz_) * f13((1, 0, 0)) - (dy_ * dz_) * f13((0, 0, 0))
        dy = 0.0 if fy else (dx_ * dz_) * f23((0, 1, 0)) - (dx_ * dz_) * f23((0, 0, 0))
        dz = 0.0 if fz else az * f33((0, 0, 0)) - az * f33((0, 0, -1))
    else:
        dz_ = W.level(m.dzc)
        ax, ay = dy_ * dz_, dx_ * dz_
        qx = lambda o: cond((FACE, CENTER, CENTER), o, -(coef * W.ddx_f(c, o)))             # noqa: E731
        qy = lambda o: cond((CENTER, FACE, CENTER), o, -(coef * W.ddy_f(c, o)))             # noqa: E731
        qz = lambda o: cond((CENTER, CENTER, FACE), o, -(coef * W.ddz_f(c, o)))             # noqa: E731
        dx = 0.0 if fx else ax * qx((1, 0, 0)) - ax * qx((0, 0, 0))
        dy = 0.0 if fy else ay * qy((0, 1, 0)) - ay * qy((0, 0, 0))
        dz = 0.0 if fz else az * qz((0, 0, 1)) - az * qz((0, 0, 0))
    vinv = 1.0 / ((dx_ * dy_) * dz_)
    Gw = W(G)
    Gw[...] = (Gw - vinv * ((dx + dy) + dz)) + 0.0
    return G


# ---------------------------------------------------------------------------------------------------------------------
# FPlane with the active-weighted average
# ---------------------------------------------------------------------------------------------------------------------
def fplane(m, imm, f, U, Gu, Gv):
    """G_u -= x_f_cross_U = -f active_weighted_ℑxyᶠᶜᶜ(v), G_v -= y_f_cross_U = f active_weighted_ℑxyᶜᶠᶜ(u) (f_plane.jl:48-52): the
    four-point average over the fraction of nodes that are not peripheral (interpolation_operators.jl:116-130); peripheral_node of the
    immersed grid counts the immersed cells"""
    fx, fy = m.flat[0], m.flat[1]
    u, v = U["u"], U["v"]
    for which, (G, q, loc) in {"u": (Gu, v, (CENTER, FACE, CENTER)), "v": (Gv, u, (FACE, CENTER, CENTER))}.items():
        r = m.default_range(LOCS[which], True)
        if r[1] < r[0] or r[3] < r[2] or r[5] < r[4]:
            continue
        W = R._Window(m, r)
        I = np.arange(r[0], r[1] + 1)[:, None, None]
        J = np.arange(r[2], r[3] + 1)[None, :, None]
        K = np.arange(r[4], r[5] + 1)[None, None, :]
        shape = (I.size, J.size, K.size)
        np_ = lambda di, dj: np.where(np.broadcast_to(imm.peripheral_node(I + di, J + dj, K, loc), shape), 0.0, 1.0)          # noqa: E731
        qv = lambda di, dj: W(q, di, dj, 0)                                                                                   # noqa: E731
        if which == "u":      # ℑyᵃᶜᵃ(ℑxᶠᵃᵃ ·): X(dj) = 0.5 (q[i-1] + q[i]); 0.5 (X(j) + X(j+1))
            X = lambda g, dj: g(0, dj) if fx else 0.5 * (g(-1, dj) + g(0, dj))                                                 # noqa: E731
            avg = lambda g: X(g, 0) if fy else 0.5 * (X(g, 0) + X(g, 1))                                                       # noqa: E731
            sign = -f
        else:                 # ℑyᵃᶠᵃ(ℑxᶜᵃᵃ ·): X(dj) = 0.5 (q[i] + q[i+1]); 0.5 (X(j-1) + X(j))
            X = lambda g, dj: g(0, dj) if fx else 0.5 * (g(0, dj) + g(1, dj))                                                  # noqa: E731
            avg = lambda g: X(g, 0) if fy else 0.5 * (X(g, -1) + X(g, 0))                                                      # noqa: E731
            sign = f
        qa, an = avg(qv), avg(np_)
        with np.errstate(divide="ignore", invalid="ignore"):
            aw = np.where(an == 0, 0.0, qa / an)
        Gw = W(G)
        Gw[...] = Gw - sign * aw


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
class ImmersedOrchestrated(R.Orchestrated):
    """Orchestrated on an immersed grid: closure = ScalarDiffusivity(ν, κ) explicit, BuoyancyTracer on tracer `buoyancy_index`, FPlane(f),
    array forcings {name: interior array}. Order of the terms as in the reference's tendency functions: advection, f × U, ∇pHY′, closure,
    forcing."""

    def __init__(self, O, grid, ntracers, nu, kappa, cell, buoyancy_index=None, fcor=None, forcing=None, bcs=None, seawater=None):
        """seawater = (g, α, β): SeawaterBuoyancy(LinearEquationOfState) on tracers 0 (T) and 1 (S) instead of a BuoyancyTracer; a
        condition's value may be an array over the two tangential extents"""
        super().__init__(O, grid, ntracers, nu, kappa, closure="numpy")
        self.bcs = {n: dict((bcs or {}).get(n, {})) for n in self.names}
        self.any_flux = any(kind == "flux" for b in self.bcs.values() for kind, _ in b.values())
        self.imm = Immersed(self.m, cell)
        self.b_index, self.fcor, self.forcing, self.seawater = buoyancy_index, fcor, dict(forcing or {}), seawater
        self.pHY = grid.zeros(LOCS["c"]) if (buoyancy_index is not None or seawater is not None) else None

    def mask(self, names):
        for n in names:
            self.imm.mask_field(self.U[n], self.loc[n])

    def update_state(self, compute_tendencies=True):
        g, U, L, O = self.g, self.U, self.L, self.O
        self.mask(self.names[3:])                          # "Mask immersed tracers" (update_nonhydrostatic_model_state.jl:22-25)
        for n in self.names:
            self._fill(n, False)
        if self.b_index is not None:
            L.oro_update_hydrostatic_pressure(g.handle, 1, O._dp(U["c%d" % self.b_index]), None, 0.0, 0.0, 0.0, O._dp(self.pHY))
        if self.seawater is not None:
            L.oro_update_hydrostatic_pressure(g.handle, 2, O._dp(U["c0"]), O._dp(U["c1"]), *[float(x) for x in self.seawater], O._dp(self.pHY))
        if not compute_tendencies:
            return
        adv = (U["u"], U["v"], U["w"])
        for n in self.names:
            advective_tendency(self.m, self.imm, n if n in "uvw" else "c", adv, U[n], G=self.Gn[n])
        if self.fcor is not None:
            fplane(self.m, self.imm, float(self.fcor), U, self.Gn["u"], self.Gn["v"])
        if self.pHY is not None:
            L.oro_add_hydrostatic_pressure_gradient(g.handle, O._dp(self.pHY), O._dp(self.Gn["u"]), O._dp(self.Gn["v"]))
        for n in self.names:
            immersed_closure_part(self.m, self.imm, n if n in "uvw" else "c", U, U[n], self.coef(n), self.Gn[n])
        for n, Fa in self.forcing.items():
            r = self.m.default_range(self.loc[n], n in "uvw")
            Gw = B._window(self.m, self.Gn[n], r)
            Gw[...] = Gw + np.asarray(Fa)[r[0] - 1:r[1], r[2] - 1:r[3], r[4] - 1:r[5]]

    def pressure_correction(self, dt):
        self.mask(self.names[:3])                          # "Mask immersed velocities" (pressure_correction.jl:10-12)
        super().pressure_correction(dt)

    def set(self, enforce_incompressibility=True, **fields):
        """set! (set_nonhydrostatic_model.jl:33-60) with "Apply a mask" (:47-49)"""
        for n, val in fields.items():
            self.g.interior(self.U[n], self.loc[n])[...] = val
        for n in self.names:
            self._fill(n, True)
        self.mask(self.names[3:])
        self.mask(self.names[:3])
        self.update_state(False)
        if enforce_incompressibility:
            self.pressure_correction(1.0)
            self.update_state(False)
