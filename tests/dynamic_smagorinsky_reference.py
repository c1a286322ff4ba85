"""Numpy restatement of Smagorinsky(coefficient = DynamicCoefficient(...)) (test infrastructure), written from the formulas and not from
any implementation (reference: Smagorinskys/dynamic_coefficient.jl, scale_invariant_operators.jl, smagorinsky.jl:92-127):

    filter(f) = ((((((6 f + f[i+1]) + f[i-1]) + f[j+1]) + f[j-1]) + f[k+1]) + f[k-1]) / 12
    Σ   = sqrt(Σ²)  over the interior, Σ² of smagorinsky_reference.strain_squared;   Σ̄ = sqrt(Σ̄²), Σ̄² the same of the FILTERED velocities
    Lᵢⱼ = filter(uᵢuⱼ at ccc) - ūᵢūⱼ at ccc:   u₁u₁ = ℑx(u u), u₁u₂ = ℑx(u) ℑy(v), ...;  ℑ(f) = 0.5 (f + f[+1]);  ū = filter(u)
    Mᵢⱼ = (2 Δf²) (filter(Σ Σᵢⱼ at ccc) - 4 (Σ̄ Σ̄ᵢⱼ at ccc)):   Σ₁₂ at ccc = ℑxy(Σ₁₂), ... nested like the squares in Σ²
    LM  = ((((L₁₁ M₁₁ + L₂₂ M₂₂) + L₃₃ M₃₃) + (2 L₁₂) M₁₂) + (2 L₁₃) M₁₃) + (2 L₂₃) M₂₃,  MM likewise with M in place of L
    cs² = 𝒥ᴹᴹ > 0 ? max(𝒥ᴸᴹ, minimum_numerator) / 𝒥ᴹᴹ : 0            νₑ = (cs² Δf²) sqrt(2 Σ²)

Two facts of the reference are part of the restatement. Σ and Σ̄ are computed over the interior and NOTHING fills their halos: filter(Σ Σᵢⱼ)
reads Σ = 0 at a neighbour outside the interior, next to a Periodic boundary as well (`sigma` returns a parent array with a zero halo; lm_mm
reads it as it is). And with LagrangianAveraging the whole parent of 𝒥 is written once, by the initialising mean; afterwards only the
interior changes, so the interpolation near a boundary reads halos that still hold that mean (`DynamicDriver`).

Averages and means are summed in the order of the library's reduction kernels (csrc/ocn_diagnostics.h: dg_reduce_rows_kernel,
dg_combine_kernel, dg_reduce_cols_kernel), restated in `ordered_average` with the terms and the metric of diagnostics_reference; the
interpolation at the displaced node is particles_reference's. Arrays are PARENT arrays indexed [i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]."""
import numpy as np

import diagnostics_reference as D
import particles_reference as P
from smagorinsky_reference import GRIDS, Metrics, _Window, _libm, case_values, make_grid, strain_squared  # noqa: F401  (re-exported)

CELLS = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]       # the order the filter adds them in


def filter_widths(m):
    """Δf per level, the scalar cube root of the C library as Metrics.df2 forms it"""
    return np.array([_libm.cbrt((m.dx * m.dy) * float(z)) for z in m.dzc])


def _shift(rng, d):
    return (rng[0] + d[0], rng[1] + d[0], rng[2] + d[1], rng[3] + d[1], rng[4] + d[2], rng[5] + d[2])


def _ring(m):
    return (0, m.N[0] + 1, 0, m.N[1] + 1, 0, m.N[2] + 1)


def filtered(m, f):
    """filter(f) on the interior plus one ring, in a parent array that is zero elsewhere"""
    W = _Window(m, _ring(m))
    s = 6 * W(f) + W(f, 1, 0, 0)
    for d in CELLS[2:]:
        s = s + W(f, *d)
    out = np.zeros_like(f)
    W(out)[...] = s / 12
    return out


def _on_interior(m, values):
    out = np.zeros(tuple(n + 2 * h for n, h in zip(m.N, m.H)), order="F")
    _Window(m, m.interior())(out)[...] = values
    return out


def sigma(m, u, v, w):
    """Σ: a ccc parent array, the interior written, the halo 0 as the reference leaves it"""
    return _on_interior(m, np.sqrt(strain_squared(m, u, v, w, m.interior())))


def sigma_bar(m, ub, vb, wb):
    """Σ̄ from the filtered velocities"""
    return _on_interior(m, np.sqrt(strain_squared(m, ub, vb, wb, m.interior())))


def strain_ccc(m, u, v, w, rng):
    """Σ₁₁, Σ₂₂, Σ₃₃, ℑxy(Σ₁₂), ℑxz(Σ₁₃), ℑyz(Σ₂₃) over the cells of rng"""
    W = _Window(m, rng)
    s11 = (W(u, 1, 0, 0) - W(u)) * m.rdx
    s22 = (W(v, 0, 1, 0) - W(v)) * m.rdy
    s33 = (W(w, 0, 0, 1) - W(w)) * (1.0 / W.level(m.dzc))
    s12 = lambda o: 0.5 * (W.ddy_f(u, o) + W.ddx_f(v, o))                # noqa: E731
    s13 = lambda o: 0.5 * (W.ddz_f(u, o) + W.ddx_f(w, o))                # noqa: E731
    s23 = lambda o: 0.5 * (W.ddz_f(v, o) + W.ddy_f(w, o))                # noqa: E731
    ixy = 0.5 * (0.5 * (s12((0, 0, 0)) + s12((1, 0, 0))) + 0.5 * (s12((0, 1, 0)) + s12((1, 1, 0))))
    ixz = 0.5 * (0.5 * (s13((0, 0, 0)) + s13((1, 0, 0))) + 0.5 * (s13((0, 0, 1)) + s13((1, 0, 1))))
    iyz = 0.5 * (0.5 * (s23((0, 0, 0)) + s23((0, 1, 0))) + 0.5 * (s23((0, 0, 1)) + s23((0, 1, 1))))
    return [s11, s22, s33, ixy, ixz, iyz]


def products_ccc(m, u, v, w, rng):
    """u₁u₁, u₂u₂, u₃u₃, u₁u₂, u₁u₃, u₂u₃ at ccc over the cells of rng"""
    W = _Window(m, rng)
    u0, u1, v0, v1, w0, w1 = W(u), W(u, 1, 0, 0), W(v), W(v, 0, 1, 0), W(w), W(w, 0, 0, 1)
    uc, vc, wc = 0.5 * (u0 + u1), 0.5 * (v0 + v1), 0.5 * (w0 + w1)
    return [0.5 * (u0 * u0 + u1 * u1), 0.5 * (v0 * v0 + v1 * v1), 0.5 * (w0 * w0 + w1 * w1), uc * vc, uc * wc, vc * wc]


def tensors(m, u, v, w, Sig=None, Sigb=None, filtered_velocities=None):
    """the six Lᵢⱼ and the six Mᵢⱼ over the interior, in the order 11, 22, 33, 12, 13, 23. Sig: Σ as a parent array (default: sigma(), zero
    halo); a test may pass one with another halo to see what the halo does"""
    rng = m.interior()
    ub, vb, wb = filtered_velocities if filtered_velocities is not None else (filtered(m, u), filtered(m, v), filtered(m, w))
    Sig = sigma(m, u, v, w) if Sig is None else Sig
    Sigb = sigma_bar(m, ub, vb, wb) if Sigb is None else Sigb
    fl, fm = [None] * 6, [None] * 6
    for q, d in enumerate(CELLS):
        r = _shift(rng, d)
        t = products_ccc(m, u, v, w, r)
        s = strain_ccc(m, u, v, w, r)
        sig = _Window(m, r)(Sig)
        for c in range(6):
            mm = sig * s[c]
            fl[c] = 6 * t[c] if q == 0 else fl[c] + t[c]
            fm[c] = 6 * mm if q == 0 else fm[c] + mm
    tb = products_ccc(m, ub, vb, wb, rng)
    sb = strain_ccc(m, ub, vb, wb, rng)
    W = _Window(m, rng)
    sigb = W(Sigb)
    c2 = 2 * W.level(m.df2)
    L = [fl[c] / 12 - tb[c] for c in range(6)]
    M = [c2 * (fm[c] / 12 - 4 * (sigb * sb[c])) for c in range(6)]
    return L, M


def contract(L, M):
    """LM and MM (dynamic_coefficient.jl:184-185)"""
    LM = L[0] * M[0] + L[1] * M[1]
    MM = M[0] * M[0] + M[1] * M[1]
    LM, MM = LM + L[2] * M[2], MM + M[2] * M[2]
    for c in (3, 4, 5):
        LM, MM = LM + (2 * L[c]) * M[c], MM + (2 * M[c]) * M[c]
    return LM, MM


def lm_mm(m, u, v, w, Sig=None, Sigb=None, filtered_velocities=None):
    """LM and MM over the interior"""
    return contract(*tensors(m, u, v, w, Sig, Sigb, filtered_velocities))


def coefficient_squared(J_LM, J_MM, minimum_numerator):
    """cs²: a select on 𝒥ᴹᴹ > 0 (the quotient is Inf or NaN in fluid at rest)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(J_MM > 0, np.maximum(J_LM, minimum_numerator) / J_MM, 0.0)


def clamping_minimum(J_LM):
    """a minimum_numerator that clamps about half of the entries of 𝒥ᴸᴹ and leaves the rest: their median"""
    return float(np.median(J_LM))


def viscosity(m, u, v, w, J_LM, J_MM, minimum_numerator):
    """νₑ over the interior; J_LM, J_MM: interior-shaped, one point along an averaged direction"""
    W = _Window(m, m.interior())
    s2 = strain_squared(m, u, v, w, m.interior())
    return (coefficient_squared(J_LM, J_MM, minimum_numerator) * W.level(m.df2)) * np.sqrt(2 * s2)


# ---------------------------------------------------------------------------------------------------------------------
# averages in the library's summation order
# ---------------------------------------------------------------------------------------------------------------------
ROWS, WAVES, LANES, THREADS = 16, 4, 64, 256


def _tree(x, width):
    """the lanes (or threads) of the last axis combined in halving steps: x[l] += x[l + w], w = width / 2 .. 1; the result is element 0"""
    x = x.copy()
    w = width // 2
    while w > 0:
        x[..., :w] = x[..., :w] + x[..., w:2 * w]
        w //= 2
    return x[..., 0]


def _sum_rows(T):
    """x reduced: T[e, r, i] -> [e]. Chunks of 16 rows; in a chunk wave w takes the rows w, w + 4, ..., lane l the points l, l + 64, ..., each
    adding in index order; the 64 lanes combine in a tree, the four waves in order; several chunks: thread t adds the chunks t, t + 256, ...
    and the 256 threads combine in a tree"""
    E, R, n0 = T.shape
    nch = (R + ROWS - 1) // ROWS
    partial = np.zeros((E, nch))
    for c in range(nch):
        lanes = np.zeros((E, WAVES, LANES))
        for wv in range(WAVES):
            for r in range(c * ROWS + wv, min(R, (c + 1) * ROWS), WAVES):
                for base in range(0, n0, LANES):
                    seg = T[:, r, base:base + LANES]
                    lanes[:, wv, :seg.shape[1]] = lanes[:, wv, :seg.shape[1]] + seg
        per_wave = _tree(lanes, LANES)
        s = per_wave[:, 0]
        for wv in range(1, WAVES):
            s = s + per_wave[:, wv]
        partial[:, c] = s
    if nch == 1:
        return partial[:, 0]
    threads = np.zeros((E, THREADS))
    for c in range(nch):
        threads[:, c % THREADS] = threads[:, c % THREADS] + partial[:, c]
    return _tree(threads, THREADS)


def ordered_sum(v, mask):
    """the sum of v (interior-shaped) over the directions of mask, size 1 along them"""
    n0, n1, n2 = v.shape
    rj, rk = bool(mask & 2), bool(mask & 4)
    if not mask & 1:                    # x kept: one thread per output element, z outer, y inner
        out = np.zeros((n0, 1 if rj else n1, 1 if rk else n2))
        for kr in range(n2 if rk else 1):
            for jr in range(n1 if rj else 1):
                out = out + _pick(v, rj, jr, rk, kr)
        return out
    # rows of an output element: r -> (jr, kr) = (r % n1, r // n1) with both reduced, else the one reduced direction
    if rj and rk:
        T = v.transpose(2, 1, 0).reshape(1, n2 * n1, n0)                 # r = kr n1 + jr
        return _sum_rows(T).reshape(1, 1, 1)
    if rj:
        T = v.transpose(2, 1, 0)                                         # [k, j, i]: output element k, rows j
        return _sum_rows(np.ascontiguousarray(T)).reshape(1, 1, n2)
    if rk:
        T = v.transpose(1, 2, 0)                                         # [j, k, i]
        return _sum_rows(np.ascontiguousarray(T)).reshape(1, n1, 1)
    T = v.transpose(2, 1, 0).reshape(n2 * n1, 1, n0)                     # output element e = ko n1 + jo, one row
    return _sum_rows(T).reshape(n2, n1).T.reshape(1, n1, n2)


def _pick(v, rj, jr, rk, kr):
    a = v[:, jr:jr + 1, :] if rj else v
    return a[:, :, kr:kr + 1] if rk else a


def ordered_average(grid, parent, mask, use_metric=None):
    """Average(field, dims = mask) of a ccc parent array as the library forms it: interior-shaped, size 1 along the averaged directions.
    use_metric None: the package's rule (the metric where a stretched z is averaged)"""
    import oldoceananigans_jl_amd as ocn
    ccc = (ocn.Center,) * 3
    if use_metric is None:
        use_metric = bool(mask & 4) and not grid.z_regular
    v, met, count = D.reduce_terms(grid, D.Operand(0, parent, None, None, None, ccc, None, ccc), mask, use_metric)
    s = ordered_sum(v, mask)
    if use_metric:
        return s / ordered_sum(np.ascontiguousarray(met), mask)
    return s / float(count)


def ordered_mean(grid, parent):
    """mean(field): the sum over the number of points, no metric"""
    return float(ordered_average(grid, parent, 7, use_metric=False)[0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the Lagrangian average (dynamic_coefficient.jl:241-345)
# ---------------------------------------------------------------------------------------------------------------------
def lagrangian_update(grid, m, u, v, w, LM, MM, J_LM_prev, J_MM_prev, dt, minimum_numerator):
    """_lagrangian_average_LM_MM! over the interior: (𝒥ᴸᴹ, 𝒥ᴹᴹ, fraction of the displacements that were clamped). J_*_prev: parent arrays"""
    import oldoceananigans_jl_amd as ocn
    W = _Window(m, m.interior())
    jl = np.maximum(W(J_LM_prev), minimum_numerator)
    jm = W(J_MM_prev)
    df = W.level(filter_widths(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        T = (1.5 * df) / np.sqrt(np.sqrt(np.sqrt(np.sqrt(jl * jm))))
        tau = dt / T
    eps = tau / (1 + tau)
    x, y, z = grid.nodes((ocn.Center,) * 3)
    dzc = W.level(m.dzc)

    def clamp(a, lim):
        return np.where(a > lim, lim, np.where(a < -lim, -lim, a))
    raw = [W(u) * dt, W(v) * dt, W(w) * dt]
    lim = [m.dx, m.dy, dzc]
    d = [clamp(a, b) for a, b in zip(raw, lim)]
    clamped = float(np.mean([np.mean(np.abs(a) > b) for a, b in zip(raw, lim)]))
    shape = W(u).shape
    X = [np.broadcast_to(x - d[0], shape).ravel(), np.broadcast_to(y - d[1], shape).ravel(), np.broadcast_to(z - d[2], shape).ravel()]
    g = P.Geometry.of_grid(grid)
    imm = P.interpolate(g, J_MM_prev, (0, 0, 0), *X).reshape(shape)
    ilm = P.interpolate(g, J_LM_prev, (0, 0, 0), *X).reshape(shape)
    J_MM = eps * MM + (1 - eps) * imm
    star = eps * LM + (1 - eps) * np.maximum(ilm, minimum_numerator)
    return np.maximum(star, minimum_numerator), J_MM, clamped


def schedule_fires(iteration, interval, offset=0):
    return (iteration - offset) % interval == 0


class DynamicDriver:
    """compute_coefficient_fields! with its bookkeeping: previous_compute_time moves on every call, the fields where the schedule fires. mask:
    the averaged directions, 0 = LagrangianAveraging. The fields are attributes: Sigma, Sigma_bar (parents), LM, MM (interior, directional),
    J_LM, J_MM (directional: interior-shaped reduced arrays; Lagrangian: parents), J_LM_prev, J_MM_prev (parents)"""

    def __init__(self, grid, mask, minimum_numerator=1e-32, interval=1, offset=0):
        self.grid, self.m, self.mask, self.jmin, self.interval, self.offset = grid, Metrics(grid), mask, minimum_numerator, interval, offset
        self.previous_time = 0.0
        self.uninitialised = True            # see restart()
        shape = tuple(n + 2 * h for n, h in zip(self.m.N, self.m.H))
        z = lambda: np.zeros(shape, order="F")                              # noqa: E731
        self.Sigma, self.Sigma_bar, self.J_LM_prev, self.J_MM_prev = z(), z(), z(), z()
        if mask:
            red = tuple(1 if mask >> d & 1 else n for d, n in enumerate(self.m.N))
            self.LM, self.MM, self.J_LM, self.J_MM = np.zeros(self.m.N), np.zeros(self.m.N), np.zeros(red), np.zeros(red)
        else:
            self.J_LM, self.J_MM = z(), z()
        self.updates = self.initialisations = 0
        self.clamped = []

    def update(self, u, v, w, time, iteration, last_dt):
        """one call of compute_coefficient_fields! with the clock (time, iteration, last_Δt)"""
        dt = time - self.previous_time
        self.previous_time = time
        if not schedule_fires(iteration, self.interval, self.offset):
            return False
        self.coefficient_update(u, v, w, dt, self.uninitialised or not np.isfinite(last_dt) or dt == 0)
        self.uninitialised = False
        return True

    def restart(self, time):
        """what setting the clock of a model does (a restored checkpoint: the 𝒥 fields are not part of it): no time has passed since the
        previous call, and the first update that fires initialises, whatever the clock says. A new driver starts like this at time 0.
        Beyond the reference, whose averaging branch would blend with 𝒥⁻ = 0 -- T⁻ = Inf, ε = 0 -- and keep 𝒥ᴹᴹ = 0 for ever"""
        self.previous_time = time
        self.uninitialised = True

    def coefficient_update(self, u, v, w, dt=0.0, initialising=True):
        m = self.m
        fv = (filtered(m, u), filtered(m, v), filtered(m, w))
        self.Sigma, self.Sigma_bar = sigma(m, u, v, w), sigma_bar(m, *fv)
        LM, MM = lm_mm(m, u, v, w, self.Sigma, self.Sigma_bar, fv)
        self.updates += 1
        if self.mask:
            self.LM, self.MM = LM, MM
            self.J_LM = ordered_average(self.grid, _on_interior(m, LM), self.mask)
            self.J_MM = ordered_average(self.grid, _on_interior(m, MM), self.mask)
            return
        self.J_LM_prev, self.J_MM_prev = self.J_LM.copy(order="F"), self.J_MM.copy(order="F")
        if initialising:
            self.initialisations += 1
            self.J_LM = np.full_like(self.J_LM, max(ordered_mean(self.grid, _on_interior(m, LM)), self.jmin))
            self.J_MM = np.full_like(self.J_MM, ordered_mean(self.grid, _on_interior(m, MM)))
            return
        jl, jm, clamped = lagrangian_update(self.grid, m, u, v, w, LM, MM, self.J_LM_prev, self.J_MM_prev, dt, self.jmin)
        self.clamped.append(clamped)
        W = _Window(m, m.interior())
        W(self.J_LM)[...] = jl
        W(self.J_MM)[...] = jm

    def interior_J(self):
        """𝒥ᴸᴹ, 𝒥ᴹᴹ shaped for viscosity()"""
        if self.mask:
            return self.J_LM, self.J_MM
        W = _Window(self.m, self.m.interior())
        return W(self.J_LM), W(self.J_MM)

    def viscosity(self, u, v, w):
        return viscosity(self.m, u, v, w, *self.interior_J(), self.jmin)
