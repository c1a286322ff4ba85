"""Numpy restatement of Lagrangian particle tracking (test infrastructure), every expression with the line of the reference it restates:

  * julia_mod            -- mod(x, y) for floats (Julia base/float.jl): rem, the sign of y on a zero, + y where the signs differ
  * fractional_index     -- index_binary_search + fractional_index (Fields/interpolate.jl:30-59)
  * fractional_indices   -- fractional_x/y/z_index (:67-83,137-188): (x - x₀) / Δ + 1 with a true division in a regular direction, the binary
                            search over the nodes of a stretched z, nothing in a Flat direction
  * interpolator         -- (i⁻, i⁺, ξ) = (unsafe_trunc, i⁻ + 1, mod(fidx, 1)) (:298-310); Flat: (1, 1, 0)
  * interpolate          -- _interpolate (:313-336): ϕ₁ … ϕ₈ as left-associated products, all eight terms, summed left to right
  * enforce              -- enforce_boundary_conditions, bounce_left, bounce_right (lagrangian_particle_advection.jl:10-46)
  * advect               -- advect_particle (:118-178) with the Cartesian metrics 1; with depths _advect_drogued_particles!
                            (drogued_dynamics.jl:57-72)
  * step                 -- step_lagrangian_particles! (LagrangianParticleTracking.jl:140-149): tracked properties first
                            (update_lagrangian_particle_properties.jl:6-36), then the move
  * ParticlesOrchestrated -- stokes_reference.StokesOrchestrated with the step after every stage's update_state! (runge_kutta_3.jl:128,144,
                            167; quasi_adams_bashforth_2.jl:108)

The restatement does NOT clamp indices: like the reference it indexes where the interpolator says, and asserts that this is inside the
parent array. tests/test_particles_host.py pins it by facts that do not depend on it. Arrays are PARENT arrays, Fortran order, indexed
[i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]; loc = (ℓx, ℓy, ℓz) with 1 = Face, 0 = Center."""
import numpy as np

import stokes_reference as S
from vertically_implicit_reference import G1, G2, G3, Z2, Z3

PERIODIC, BOUNDED, FLAT = 0, 1, 3
CENTER, FACE = 0, 1


def julia_mod(x, y):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        r = np.fmod(x, y)
        return np.where(r == 0, np.copysign(r, y), np.where((r > 0) != (y > 0), r + y, r))


def index_binary_search(vec, val, N):
    """(i₁, i₂), 1-based (interpolate.jl:30-46)"""
    low, high = 0, N - 1
    while low + 1 < high:
        mid = int((low + high) / 2)                      # middle_point: unsafe_trunc(Int, (l + h) / 2)
        if vec[mid] == val:
            return mid + 1, mid + 1
        elif vec[mid] < val:
            low = mid
        else:
            high = mid
    return low + 1, high + 1


def fractional_index(val, vec, N):
    """interpolate.jl:48-59"""
    i1, i2 = index_binary_search(vec, val, N)
    x1, x2 = vec[i1 - 1], vec[i2 - 1]
    if i1 == i2:
        return np.float64(i1)
    return np.float64(i2 - i1) / (x2 - x1) * (val - x1) + np.float64(i1)


class Geometry:
    """what the index computation needs of a grid: per direction N, H, topology code, the first Face node, the first Center node, Δ, the
    walls xᴸ = face 1 and xᴿ = face N + 1; zf / zc: the node vectors of a stretched z (else None)"""

    def __init__(self, N, H, topo, f0, c0, d, xL, xR, zf=None, zc=None):
        self.N, self.H, self.topo = tuple(N), tuple(H), tuple(topo)
        self.f0, self.c0, self.d, self.xL, self.xR = (tuple(float(a) for a in v) for v in (f0, c0, d, xL, xR))
        self.zf = None if zf is None else np.asarray(zf, dtype=np.float64)
        self.zc = None if zc is None else np.asarray(zc, dtype=np.float64)

    @classmethod
    def of_grid(cls, grid):
        """from a RectilinearGrid of the package (host metadata only: no device is touched)"""
        import oldoceananigans_jl_amd as ocn
        codes = {ocn.Periodic: PERIODIC, ocn.Bounded: BOUNDED, ocn.Flat: FLAT}
        topo = [codes[t] for t in grid.topology]
        N, H = grid.size, grid.halo_size
        F, Cn = (grid.xᶠᵃᵃ, grid.yᵃᶠᵃ, grid.zᵃᵃᶠ), (grid.xᶜᵃᵃ, grid.yᵃᶜᵃ, grid.zᵃᵃᶜ)
        at = lambda a, d, i: float(a[0]) if topo[d] == FLAT else float(a[i - 1 + H[d]])               # noqa: E731
        f0 = [at(F[d], d, 1) for d in range(3)]
        c0 = [at(Cn[d], d, 1) for d in range(3)]
        xR = [at(F[d], d, N[d] + 1) for d in range(3)]
        dz = 1.0 if topo[2] == FLAT else float(grid.Δzᵃᵃᶜ[H[2]])
        zf = zc = None
        if not grid.z_regular:
            zf, zc = grid.zᵃᵃᶠ[H[2]:H[2] + N[2] + 1], grid.zᵃᵃᶜ[H[2]:H[2] + N[2]]
        return cls(N, H, topo, f0, c0, (grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, dz), f0, xR, zf, zc)

    def length(self, d):
        return self.xR[d] - self.xL[d]


def fractional_indices(g, d, face, x):
    """the fractional index of every coordinate in x along direction d at a Face or a Center; None along a Flat direction"""
    if g.topo[d] == FLAT:
        return None
    x = np.asarray(x, dtype=np.float64)
    tab = (g.zf if face else g.zc) if d == 2 else None
    if tab is not None:
        n = g.N[2] + 1 if face else g.N[2]
        return np.array([fractional_index(v, tab, n) for v in x], dtype=np.float64)
    x0 = g.f0[d] if face else g.c0[d]
    return (x - x0) / g.d[d] + 1.0


def interpolator(fidx, n=None):
    """(i⁻, i⁺, ξ) (interpolate.jl:298-310); fidx None: interpolator(::Nothing) = (1, 1, 0) for n points"""
    if fidx is None:
        return np.ones(n, dtype=np.int64), np.ones(n, dtype=np.int64), np.zeros(n)
    im = np.trunc(fidx).astype(np.int64)
    return im, im + 1, julia_mod(fidx, 1.0)


def interpolators(g, loc, x, y, z):
    X = (x, y, z)
    return [interpolator(fractional_indices(g, d, loc[d] == FACE, X[d]), len(np.atleast_1d(x))) for d in range(3)]


def _interpolate(g, data, ix, iy, iz):
    """_interpolate (interpolate.jl:322-336)"""
    (i0, i1, xi), (j0, j1, eta), (k0, k1, zeta) = ix, iy, iz
    H = g.H

    def at(i, j, k):
        I, J, K = i - 1 + H[0], j - 1 + H[1], k - 1 + H[2]
        for a, n in ((I, data.shape[0]), (J, data.shape[1]), (K, data.shape[2])):
            assert a.min() >= 0 and a.max() < n, "the restatement indexes like the reference: a corner outside the parent array"
        return data[I, J, K]
    p1 = ((1 - xi) * (1 - eta)) * (1 - zeta)
    p2 = ((1 - xi) * (1 - eta)) * zeta
    p3 = ((1 - xi) * eta) * (1 - zeta)
    p4 = ((1 - xi) * eta) * zeta
    p5 = (xi * (1 - eta)) * (1 - zeta)
    p6 = (xi * (1 - eta)) * zeta
    p7 = (xi * eta) * (1 - zeta)
    p8 = (xi * eta) * zeta
    s = p1 * at(i0, j0, k0)
    s = s + p2 * at(i0, j0, k1)
    s = s + p3 * at(i0, j1, k0)
    s = s + p4 * at(i0, j1, k1)
    s = s + p5 * at(i1, j0, k0)
    s = s + p6 * at(i1, j0, k1)
    s = s + p7 * at(i1, j1, k0)
    s = s + p8 * at(i1, j1, k1)
    return s


def interpolate(g, data, loc, x, y, z):
    """interpolate(X, field, loc, grid) (interpolate.jl:272-282)"""
    x, y, z = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (x, y, z))
    return _interpolate(g, data, *interpolators(g, loc, x, y, z))


def enforce(topo, x, xL, xR, Cr):
    """enforce_boundary_conditions (lagrangian_particle_advection.jl:29-46)"""
    x = np.asarray(x, dtype=np.float64)
    if topo == BOUNDED:
        xi = xR - Cr * (x - xR)
        left = np.where(xi < xL, xL, xi)                 # bounce_left (:10-14)
        xi = xL + Cr * (xL - x)
        right = np.where(xi > xR, xR, xi)                # bounce_right (:16-20)
        return np.where(x > xR, left, np.where(x < xL, right, x))
    if topo == PERIODIC:
        return np.where(x > xR, xL + julia_mod(x - xR, xR - xL), np.where(x < xL, xR - julia_mod(xL - x, xR - xL), x))
    return x


LOC_U, LOC_V, LOC_W, LOC_C = (FACE, CENTER, CENTER), (CENTER, FACE, CENTER), (CENTER, CENTER, FACE), (CENTER, CENTER, CENTER)


def advect(g, x, y, z, u, v, w, dt, Cr, depths=None):
    """advect_particle for every particle -> (x⁺, y⁺, z⁺); depths: the velocities at (x, y, depths), z unchanged"""
    x, y, z = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (x, y, z))
    za = z if depths is None else np.asarray(depths, dtype=np.float64)
    up = interpolate(g, u, LOC_U, x, y, za)
    vp = interpolate(g, v, LOC_V, x, y, za)
    wp = interpolate(g, w, LOC_W, x, y, za)
    xn = enforce(g.topo[0], x + (1 * up) * dt, g.xL[0], g.xR[0], Cr)
    yn = enforce(g.topo[1], y + (1 * vp) * dt, g.xL[1], g.xR[1], Cr)
    zn = z.copy() if depths is not None else enforce(g.topo[2], z + wp * dt, g.xL[2], g.xR[2], Cr)
    return xn, yn, zn


def step(g, P, tracked, velocities, dt, Cr, depths=None):
    """step_lagrangian_particles!: P = {"x", "y", "z", properties...} updated in place; tracked = [(property, parent array, loc)]"""
    for name, data, loc in tracked:
        P[name] = interpolate(g, data, loc, P["x"], P["y"], P["z"])
    P["x"], P["y"], P["z"] = advect(g, P["x"], P["y"], P["z"], *velocities, dt, Cr, depths)
    return P


def face_distance(g, P):
    """the smallest distance of any particle to a face of the domain over the directions that are not Flat"""
    best = np.inf
    for d, n in enumerate("xyz"):
        if g.topo[d] != FLAT:
            best = min(best, float(np.min(P[n] - g.xL[d])), float(np.min(g.xR[d] - P[n])))
    return best


class ParticlesOrchestrated(S.StokesOrchestrated):
    """StokesOrchestrated with particles = {"x", "y", "z", properties...}: the step follows the update_state! of every RK3 stage, with γ¹Δt,
    (γ² + ζ²)Δt and the uncorrected (γ³ + ζ³)Δt, and the one of an AB2 step with Δt. tracked = {property: field name "u" | "v" | "w" |
    "c<n>"}. min_face_distance: the smallest face_distance seen before or after any move."""

    def __init__(self, O, grid, ntracers, nu, kappa, geometry=None, particles=None, restitution=1.0, depths=None, tracked=None, **kw):
        super().__init__(O, grid, ntracers, nu, kappa, **kw)
        self.geometry, self.restitution, self.depths = geometry, restitution, depths
        self.P = {n: np.array(a, dtype=np.float64) for n, a in particles.items()}
        self.tracked = dict(tracked or {})
        self._pending = []
        self.min_face_distance = face_distance(geometry, self.P)

    def update_state(self, compute_tendencies=True):
        super().update_state(compute_tendencies)
        if self._pending:
            dt = self._pending.pop(0)
            if dt is not None:
                tracked = [(prop, self.U[name], self.loc[name]) for prop, name in self.tracked.items()]
                velocities = self.total if self.total is not None else tuple(self.U[n] for n in "uvw")
                step(self.geometry, self.P, tracked, velocities, dt, self.restitution, self.depths)
                self.min_face_distance = min(self.min_face_distance, face_distance(self.geometry, self.P))

    def time_step(self, dt):
        first = [None] if self.iteration == 0 else []
        self._pending = first + [dt * G1, dt * (G2 + Z2), dt * (G3 + Z3)]
        super().time_step(dt)
        assert not self._pending

    def time_step_ab2(self, dt, **kw):
        first = [None] if self.iteration == 0 else []
        self._pending = first + [dt]
        super().time_step_ab2(dt, **kw)
        assert not self._pending
