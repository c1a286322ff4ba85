"""Numpy restatement of OpenBoundaryCondition(value; scheme = PerturbationAdvection(inflow_timescale, outflow_timescale)) and of the
mass-flux correction of a NonhydrostaticModel with such sides (test infrastructure), every expression with the line of the reference it
restates:

  * step_boundary       -- step_right_boundary! / step_left_boundary! (BoundaryConditions/perturbation_advection.jl:71-117)
  * step_side           -- _fill_west_halo! .. _fill_top_halo! for a PAOBC (:119-180) on a parent array
  * mass_flux           -- west_mass_flux .. top_mass_flux (Models/NonhydrostaticModels/boundary_mass_fluxes.jl:47-55)
  * mass_inflow         -- open_boundary_mass_inflow with initialize_boundary_mass_flux's dispatch (:57-79, 181-198)
  * enforce             -- enforce_open_boundary_mass_conservation! (:200-239)
  * OpenBoundaryOrchestrated -- vertically_implicit_reference.Orchestrated with scheme sides stepped (not imposed) in the open fill and the
                           correction between the velocity fill and the source term (pressure_correction.jl:12-14)

The step is a chain of elementwise IEEE float64 operations in the stated association order: a device result can be compared with
np.array_equal. The sums of the flux integrals are np.sum's; their order is not the reference's (nor the device's), which the round-off
bound `flux_bound` covers. Arrays are PARENT arrays (halos included), Fortran order, as in vertically_implicit_reference."""
import numpy as np

from vertically_implicit_reference import BOUNDED, EPS, LOCS, Orchestrated

SIDES = ("west", "east", "south", "north", "bottom", "top")
NORMAL = {"west": "u", "east": "u", "south": "v", "north": "v", "bottom": "w", "top": "w"}


def step_boundary(uB, uA, ubar, dX, inflow_timescale, outflow_timescale, last_stage_dt, right):
    """the new boundary value from uᵢⁿ = uB, uᵢ₋₁ⁿ⁺¹ = uA and ūⁿ⁺¹ = ubar (arrays or numbers)"""
    dt = 0.0 if np.isinf(last_stage_dt) else float(last_stage_dt)                      # :75-76, :99-100
    uB, uA = np.asarray(uB, dtype=np.float64), np.asarray(uA, dtype=np.float64)
    ubar = np.broadcast_to(np.asarray(ubar, dtype=np.float64), uB.shape)
    c = dt / dX * ubar                                                                 # Δt / ΔX * ūⁿ⁺¹
    with np.errstate(divide="ignore", invalid="ignore"):
        if right:
            U = np.maximum(0.0, np.minimum(1.0, c))                                    # :81
            tau = np.where(ubar >= 0, outflow_timescale, inflow_timescale)             # :84
            tt = dt / tau                                                              # :85
            relaxed = (uB + U * uA + ubar * tt) / (1 + tt + U)                         # :87
        else:
            U = np.minimum(0.0, np.maximum(-1.0, c))                                   # :105
            tau = np.where(ubar <= 0, outflow_timescale, inflow_timescale)             # :108
            tt = dt / tau                                                              # :109
            relaxed = (uB - U * uA + ubar * tt) / (1 + tt - U)                         # :111
    return np.where(tau == 0, ubar, relaxed)                                           # :88, :112


def _planes(m, parent, side):
    """views (boundary plane, boundary-adjacent plane) of the wall-normal velocity's parent array over the interior extents of the two
    tangential directions, and ΔX at the boundary index"""
    d, right = SIDES.index(side) // 2, SIDES.index(side) % 2
    N, H = m.N, m.H
    sl = [slice(H[q], H[q] + N[q]) for q in range(3)]
    iB = H[d] + (N[d] if right else 0)                       # i = N + 1 | 1
    iA = H[d] + (N[d] - 1 if right else 1)                   # i = N     | 2
    slB, slA = list(sl), list(sl)
    slB[d], slA[d] = iB, iA
    # Δxᶠᶜᶜ(i, j, k), Δyᶜᶠᶜ, Δzᶜᶜᶠ at the boundary index (:124,134,145,155,166,176)
    dX = m.dx if d == 0 else (m.dy if d == 1 else float(m.dzf[(N[2] if right else 0) + H[2]]))
    return parent[tuple(slB)], parent[tuple(slA)], dX


def step_side(m, parent, side, ubar, inflow_timescale, outflow_timescale, last_stage_dt):
    """_fill_<side>_halo!(..., bc::PAOBC, ...) over the face, in place"""
    B, A, dX = _planes(m, parent, side)
    B[...] = step_boundary(B.copy(), A, ubar, dX, inflow_timescale, outflow_timescale, last_stage_dt, SIDES.index(side) % 2 == 1)
    return parent


def face_areas(m, side):
    """Axᶠᶜᶜ = Δy Δzᶜ, Ayᶜᶠᶜ = Δx Δzᶜ, Azᶜᶜᶠ = Δx Δy over the face (the two tangential interior extents)"""
    d = SIDES.index(side) // 2
    Nx, Ny, Nz = m.N
    dzc = m.dzc[m.H[2]:m.H[2] + Nz]
    if d == 0:
        return np.broadcast_to((m.dy * dzc)[None, :], (Ny, Nz))
    if d == 1:
        return np.broadcast_to((m.dx * dzc)[None, :], (Nx, Nz))
    return np.full((Nx, Ny), m.dx * m.dy)


def face_area(m, side):
    """get_west_area .. get_top_area (:11-45)"""
    return float(np.sum(face_areas(m, side)))


def mass_flux(m, parent, side):
    """west_mass_flux(u) = Field(Integral(view(u, 1, :, :), dims = (2, 3))) and its five siblings (:47-55)"""
    B, _, _ = _planes(m, parent, side)
    return float(np.sum(B * face_areas(m, side)))


def abs_flux(m, parent, side):
    B, _, _ = _planes(m, parent, side)
    return float(np.sum(np.abs(B * face_areas(m, side))))


def _is_wall(m, side):
    return m.topo[SIDES.index(side) // 2] == BOUNDED


def mass_inflow(m, U, conditions, schemes):
    """open_boundary_mass_inflow (:181-198). conditions: side -> number | array | None of the wall-normal velocity's Open condition (None or
    missing: no Open condition, flux zero); schemes: side -> (inflow_timescale, outflow_timescale) for the sides that carry one. A scheme
    face and an array-valued imposed face are integrated (:57-62), a constant imposed face contributes condition * area (:71-76)."""
    total = 0.0
    for side in SIDES:
        cond = conditions.get(side)
        if cond is None or not _is_wall(m, side):
            continue
        if side in schemes or isinstance(cond, np.ndarray):
            flux = mass_flux(m, U[NORMAL[side]], side)
        else:
            flux = float(cond) * face_area(m, side)
        total = total + flux if SIDES.index(side) % 2 == 0 else total - flux       # :188-195
    return total


def enforce(m, U, conditions, schemes):
    """enforce_open_boundary_mass_conservation! (:224-239), in place; returns A⁻¹ ∮u dA (None without a scheme side, :216)"""
    sides = [s for s in SIDES if s in schemes and conditions.get(s) is not None and _is_wall(m, s)]
    if not sides:
        return None
    A = 0.0
    for side in sides:
        A += face_area(m, side)                                                     # total_area_scheme_boundaries (:109-149)
    corr = mass_inflow(m, U, conditions, schemes) / A                               # :227-230
    for side in sides:
        B, _, _ = _planes(m, U[NORMAL[side]], side)
        if SIDES.index(side) % 2 == 0:
            B[...] = B - corr                                                       # :200-202
        else:
            B[...] = B + corr                                                       # :208-210
    return corr


def flux_bound(m, U, conditions, schemes):
    """round-off bound of the sums involved: 4 n_face_points eps Σ|u A| over the open faces"""
    n, s = 0, 0.0
    for side in SIDES:
        cond = conditions.get(side)
        if cond is None or not _is_wall(m, side):
            continue
        B, _, _ = _planes(m, U[NORMAL[side]], side)
        n += B.size
        if side in schemes or isinstance(cond, np.ndarray):
            s += abs_flux(m, U[NORMAL[side]], side)
        else:
            s += abs(float(cond)) * face_area(m, side)
    return 4 * n * EPS * s


class OpenBoundaryOrchestrated(Orchestrated):
    """Orchestrated with bcs[name][side] = ("open", value) and schemes = {side: (inflow_timescale, outflow_timescale)} on the wall-normal
    velocities. A fill with fill_open_bcs = true steps the scheme sides with clock.last_stage_Δt instead of imposing the value; update_state!
    (fill_open_bcs = false) leaves them alone; compute_pressure_correction! corrects the mass flux between the velocity fill and the source
    term."""

    def __init__(self, O, grid, ntracers, nu, kappa, closure="oracle", bcs=None, schemes=None):
        super().__init__(O, grid, ntracers, nu, kappa, closure=closure, bcs=bcs)
        self.schemes = dict(schemes or {})
        for side in self.schemes:
            assert self.bcs[NORMAL[side]].get(side, ("default", 0.0))[0] == "open", side

    def conditions(self):
        return {side: self.bcs[NORMAL[side]][side][1] for side in SIDES if self.bcs[NORMAL[side]].get(side, ("default", 0.0))[0] == "open"}

    def _fill(self, n, fill_open):
        sides = [s for s in self.schemes if NORMAL[s] == n] if fill_open else []
        if not sides:
            return super()._fill(n, fill_open)
        # the oracle's fill imposes the value on every Open side; the scheme sides' previous boundary values -- the scheme's state -- are
        # kept aside and stepped from them afterwards. The tangential halos of a boundary plane (the only other cells that see the
        # imposed value) are written again by update_state!'s fill before anything reads them.
        before = {s: _planes(self.m, self.U[n], s)[0].copy() for s in sides}
        super()._fill(n, True)
        for s in sides:
            B, _, _ = _planes(self.m, self.U[n], s)
            B[...] = before[s]
            tin, tout = self.schemes[s]
            step_side(self.m, self.U[n], s, self.bcs[n][s][1], tin, tout, self.last_stage_dt)

    def pressure_correction(self, dt):
        """compute_pressure_correction! + make_pressure_correction! (pressure_correction.jl:8-53)"""
        g, U, L = self.g, self.U, self.L
        for n in ("u", "v", "w"):
            self._fill(n, True)                                                     # :12
        enforce(self.m, U, self.conditions(), self.schemes)                         # :14
        L.oro_compute_source_term(g.handle, self.O._dp(U["u"]), self.O._dp(U["v"]), self.O._dp(U["w"]), L.oro_poisson_rhs(self.solver.handle),
                                  int(self.solver.kind == 1))
        self.solver.solve(self.p)
        g.fill_halo_regions(self.p, LOCS["c"])
        g.pressure_correct(U["u"], U["v"], U["w"], self.p)
        L.oro_scale_parent(g.handle, self.O._dp(self.p), self.O._i3(LOCS["c"]), max(EPS, dt))


def integrated_divergence(m, U):
    """Σ (∂x u + ∂y v + ∂z w) V over the cells = Integral(∂x(u) + ∂y(v) + ∂z(w)) (test_boundary_conditions_integration.jl:176-181)"""
    Nx, Ny, Nz = m.N
    Hx, Hy, Hz = m.H
    c = (slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hz, Hz + Nz))
    sh = lambda d: tuple(slice(s.start + (1 if q == d else 0), s.stop + (1 if q == d else 0)) for q, s in enumerate(c))       # noqa: E731
    dzc = m.dzc[Hz:Hz + Nz][None, None, :]
    u, v, w = U["u"], U["v"], U["w"]
    div = np.zeros((Nx, Ny, Nz))
    if not m.flat[0]:
        div = div + (u[sh(0)] - u[c]) / m.dx
    if not m.flat[1]:
        div = div + (v[sh(1)] - v[c]) / m.dy
    if not m.flat[2]:
        div = div + (w[sh(2)] - w[c]) / dzc
    return float(np.sum(div * ((m.dx * m.dy) * dzc)))
