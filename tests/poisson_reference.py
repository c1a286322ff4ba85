"""A direct solve of the model's discrete pressure Poisson equation in 80-bit long double: plain NumPy, no device code, nothing of the oracle.

The discrete problem (solve_for_pressure.jl:12-42, pressure_correction.jl:31-37): on cell centres of a RectilinearGrid with regular x, y and a
regular or stretched z,

    δx(δx p) / Δx² + δy(δy p) / Δy² + δz(δz p / Δzᶠ) / Δzᶜ = R,      R = ∇·U,

Periodic directions wrap, Bounded directions have no-flux walls, Flat directions carry nothing. The Fourier-tridiagonal solver takes the
equation times Δzᶜ (`weighted`). The operator is singular (constants); both solvers of the reference return the solution whose arithmetic
mean over all cells is zero (fft_based_poisson_solver.jl:95-125 zeroes the (0, 0, 0) mode, which for DFT and DCT-II alike is the plain sum;
fourier_tridiagonal_poisson_solver.jl:212-239 subtracts mean(ϕ)). That solution is unique, so a field that satisfies the equation to
long-double round-off (`residual`) and has zero mean IS the answer, by whatever route it was computed: every user asserts `certify` first.

The route taken here: explicit eigenvector matrices per transformed direction (a DFT matrix for Periodic, the DCT-II basis for Bounded), built
with long-double cos / sin of exactly reduced angles, applied as dense matrix products (N x cells each); z is a third eigen-direction on the
unweighted equation and a Thomas sweep over k, vectorised over (i, j), on the weighted one."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).eps < 2e-19, "this reference needs an extended-precision long double (x86-64: 80 bits)"
PI = 4 * np.arctan(LD(1))
EPS = float(np.finfo(np.float64).eps)


class Geometry:
    """the numbers of the grid the equation needs: size, topology ("Periodic" | "Bounded" | "Flat" per direction), halo, and the float64
    spacings as the grid constructors produce them (x, y on (0, 1); z regular on an interval of length 1, or stretched-Bounded with explicit
    faces: Δzᶜ_k = F_{k+1} - F_k, Δzᶠ_k = C_k - C_{k-1} of the centres C_k = (F_{k+1} + F_k) / 2, all in float64 -- grid_generation.jl:34-95).
    The tests compare `dzc` / `dzf` with the arrays of the grid they run on, bit for bit."""

    def __init__(self, size, topology, z_faces=None, halo=(3, 3, 3)):
        self.N = tuple(int(n) for n in size)
        self.topo = tuple(topology)
        assert all(t in ("Periodic", "Bounded", "Flat") for t in self.topo)
        assert all(n == 1 for n, t in zip(self.N, self.topo) if t == "Flat")
        self.H = tuple(0 if t == "Flat" else int(h) for h, t in zip(halo, self.topo))
        self.dx = LD(np.float64(1.0) / np.float64(self.N[0]))
        self.dy = LD(np.float64(1.0) / np.float64(self.N[1]))
        Nz = self.N[2]
        self.z_regular = z_faces is None
        if z_faces is None:
            dz = np.float64(1.0) / np.float64(Nz)
            self.dzc = np.full(Nz, dz).astype(LD)
            self.dzf = np.full(Nz + 1, dz).astype(LD)           # face k lies below cell k; k = 0 .. Nz
        else:
            assert self.topo[2] == "Bounded"
            F = np.asarray(z_faces, dtype=np.float64)
            assert F.shape == (Nz + 1,) and np.all(np.diff(F) > 0)
            Cc = (F[1:] + F[:-1]) / 2
            dzf = np.empty(Nz + 1)
            dzf[1:Nz] = Cc[1:] - Cc[:-1]
            dzf[0], dzf[Nz] = F[1] - F[0], F[Nz] - F[Nz - 1]     # the walls: no flux crosses them, the value is never used
            self.dzc = (F[1:] - F[:-1]).astype(LD)
            self.dzf = dzf.astype(LD)

    def spacing(self, d):
        """(Δᶜ over the N cells, Δᶠ over the N + 1 faces) of direction d as long-double vectors"""
        if d == 2:
            return self.dzc, self.dzf
        h = self.dx if d == 0 else self.dy
        return np.full(self.N[d], h, dtype=LD), np.full(self.N[d] + 1, h, dtype=LD)

    def interior(self, parent, loc):
        """the interior of a haloed parent array at `loc` (a string of "f" / "c" per direction): N + 1 faces in a Bounded direction"""
        sl = tuple(slice(self.H[d], self.H[d] + self.N[d] + (1 if loc[d] == "f" and self.topo[d] == "Bounded" else 0)) for d in range(3))
        return parent[sl]


def _along(v, d):
    """a vector laid along direction d of a 3-D array"""
    shape = [1, 1, 1]
    shape[d] = -1
    return np.asarray(v).reshape(shape)


def _face_difference(geom, parent, d):
    """δ of a face-located haloed parent along its own direction d, on the cell centres of the interior: U[i + 1] - U[i]. The upper neighbour
    of the last cell is the first halo cell of a Periodic direction and the wall face N + 1 of a Bounded one -- both inside the parent"""
    N, H = geom.N, geom.H
    if geom.topo[d] == "Flat":
        return np.zeros(N, dtype=LD)
    lo = tuple(slice(H[q], H[q] + N[q]) for q in range(3))
    hi = tuple(slice(H[q] + (q == d), H[q] + N[q] + (q == d)) for q in range(3))
    A = np.asarray(parent, dtype=LD)
    return A[hi] - A[lo]


def source_term(geom, u, v, w, weighted):
    """the discrete divergence of the haloed velocity parents on the interior; times Δzᶜ when `weighted` (the Fourier-tridiagonal solver's
    right-hand side, solve_for_pressure.jl:36-42)"""
    R = _face_difference(geom, u, 0) / geom.dx + _face_difference(geom, v, 1) / geom.dy + _face_difference(geom, w, 2) / _along(geom.dzc, 2)
    return R * _along(geom.dzc, 2) if weighted else R


def _dft_matrix(N):
    """F[k, j] = exp(-2πi jk / N) with jk reduced mod N in integers, so the angle is exact to long-double round-off at every entry"""
    jk = np.outer(np.arange(N), np.arange(N)) % N
    ang = 2 * PI * jk.astype(LD) / LD(N)
    return (np.cos(ang) - 1j * np.sin(ang)).astype(CLD)


def _dct_matrix(N):
    """C[k, i] = cos(π (i + 1/2) k / N), the DCT-II basis: eigenvectors of the second difference with no-flux walls"""
    m = np.outer(np.arange(N), 2 * np.arange(N) + 1) % (4 * N)
    return np.cos(PI * m.astype(LD) / LD(2 * N))


def _eigenvalues(N, topo, h):
    k = np.arange(N).astype(LD)
    if topo == "Periodic":
        return (2 * np.cos(2 * PI * k / LD(N)) - 2) / (h * h)
    if topo == "Bounded":
        return (2 * np.cos(PI * k / LD(N)) - 2) / (h * h)
    return np.zeros(N, dtype=LD)


def _apply(M, A, d):
    """M applied along direction d of A"""
    return np.moveaxis(np.tensordot(M, A, axes=(1, d)), 0, d)


def _transforms(N, topo):
    """(forward, backward) matrices of one direction; None for Flat"""
    if topo == "Periodic":
        F = _dft_matrix(N)
        return F, np.conj(F) / LD(N)
    if topo == "Bounded":
        Cm = _dct_matrix(N)
        wk = np.full(N, LD(2) / LD(N))
        wk[0] = LD(1) / LD(N)
        return Cm.astype(CLD), (Cm.T * wk[None, :]).astype(CLD)
    return None, None


def solve(R, geom, weighted):
    """the zero-arithmetic-mean solution of the discrete Poisson equation with right-hand side R (Δzᶜ-weighted when `weighted`), as a real
    long-double array. `weighted` = False needs a regular z (the FFT-based solver's condition)."""
    N = geom.N
    dirs = (0, 1) if weighted else (0, 1, 2)
    assert weighted or geom.z_regular
    if weighted:
        assert geom.topo[2] == "Bounded"
    A = np.asarray(R, dtype=LD).astype(CLD)
    back = {}
    lam = []
    for d in dirs:
        fwd, back[d] = _transforms(N[d], geom.topo[d])
        if fwd is not None:
            A = _apply(fwd, A, d)
        lam.append(_eigenvalues(N[d], geom.topo[d], geom.spacing(d)[0][0]))
    if not weighted:
        L = _along(lam[0], 0) + _along(lam[1], 1) + _along(lam[2], 2)
        L[0, 0, 0] = 1
        A = A / L
        A[0, 0, 0] = 0
    else:
        # rows of the column (i, j): a_k p_{k-1} + d_k p_k + c_k p_{k+1} = R_k with a_k = 1 / Δzᶠ_k, c_k = 1 / Δzᶠ_{k+1} (zero at the walls) and
        # d_k = (λx + λy) Δzᶜ_k - a_k - c_k; the singular (0, 0) column gets its first row replaced by the identity
        Nz = N[2]
        Lxy = (_along(lam[0], 0) + _along(lam[1], 1))[:, :, 0]
        a = np.zeros(Nz, dtype=LD)
        c = np.zeros(Nz, dtype=LD)
        a[1:] = 1 / geom.dzf[1:Nz]
        c[:-1] = 1 / geom.dzf[1:Nz]
        diag = Lxy[:, :, None] * _along(geom.dzc, 2) - _along(a + c, 2)
        upper = np.broadcast_to(_along(c, 2), diag.shape).copy()
        diag[0, 0, 0], upper[0, 0, 0], A[0, 0, 0] = 1, 0, 0
        # Thomas sweep over k, every (i, j) at once
        cp = np.empty_like(diag)
        P = np.empty_like(A)
        beta = diag[:, :, 0].copy()
        P[:, :, 0] = A[:, :, 0] / beta
        for k in range(1, Nz):
            cp[:, :, k] = upper[:, :, k - 1] / beta
            beta = diag[:, :, k] - a[k] * cp[:, :, k]
            P[:, :, k] = (A[:, :, k] - a[k] * P[:, :, k - 1]) / beta
        for k in range(Nz - 2, -1, -1):
            P[:, :, k] -= cp[:, :, k + 1] * P[:, :, k + 1]
        A = P
    for d in dirs:
        if back[d] is not None:
            A = _apply(back[d], A, d)
    p = np.ascontiguousarray(A.real)
    return p - p.mean(dtype=LD)


def _laplacian_term(geom, p, d):
    """δ(δp / Δᶠ) / Δᶜ along direction d: Periodic wraps, Bounded has no flux through the walls, Flat has none at all"""
    topo, n = geom.topo[d], geom.N[d]
    if topo == "Flat":
        return np.zeros_like(p)
    dc, df = geom.spacing(d)
    flux = np.zeros(tuple(n + 1 if q == d else geom.N[q] for q in range(3)), dtype=LD)       # on the N + 1 faces
    inner = tuple(slice(1, n) if q == d else slice(None) for q in range(3))
    up = tuple(slice(1, n) if q == d else slice(None) for q in range(3))
    dn = tuple(slice(0, n - 1) if q == d else slice(None) for q in range(3))
    flux[inner] = (p[up] - p[dn]) / _along(df[1:n], d)
    if topo == "Periodic":
        first = tuple(slice(0, 1) if q == d else slice(None) for q in range(3))
        last = tuple(slice(n - 1, n) if q == d else slice(None) for q in range(3))
        wall = (p[first] - p[last]) / df[0]
        flux[tuple(slice(0, 1) if q == d else slice(None) for q in range(3))] = wall
        flux[tuple(slice(n, n + 1) if q == d else slice(None) for q in range(3))] = wall
    hi = tuple(slice(1, n + 1) if q == d else slice(None) for q in range(3))
    lo = tuple(slice(0, n) if q == d else slice(None) for q in range(3))
    return (flux[hi] - flux[lo]) / _along(dc, d)


def residual(p, R, geom, weighted):
    """the discrete Laplacian of p minus R, element-wise in long double (times Δzᶜ first when R is the weighted source)"""
    p = np.asarray(p, dtype=LD)
    lap = _laplacian_term(geom, p, 0) + _laplacian_term(geom, p, 1) + _laplacian_term(geom, p, 2)
    if weighted:
        lap = lap * _along(geom.dzc, 2)
    return lap - np.asarray(R, dtype=LD)


def relative_residual(p, R, geom, weighted):
    """max |∇²p - R| / max |R|"""
    return float(np.abs(residual(p, R, geom, weighted)).max() / np.abs(np.asarray(R, dtype=LD)).max())


def certify(p, R, geom, weighted, bound=1e-15):
    """the line every use of a reference solution asserts first: it satisfies the discrete equation to 1e-15 max|R| and has zero mean, so
    (the zero-mean solution being unique) it is the answer. Returns the relative residual."""
    r = relative_residual(p, R, geom, weighted)
    assert r <= bound, ("the long-double reference does not satisfy its own equation", geom.N, geom.topo, r)
    assert abs(float(p.mean(dtype=LD))) <= 1e-18 * float(np.abs(p).max()), "the long-double reference is not mean-free"
    return r


def rel_err(a, ref):
    """max |a - ref| / max |ref| with the difference taken in long double"""
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(a, dtype=LD) - ref).max() / np.abs(ref).max())


def project(geom, u, v, w, p, dt=1):
    """the interiors of u, v, w (N + 1 faces in a Bounded direction) minus Δt ∂p on the faces (pressure_correction.jl:31-37), in long double;
    wall faces are left untouched, a Flat direction has no gradient"""
    p = np.asarray(p, dtype=LD)
    out = []
    for d, (U, loc) in enumerate(((u, "fcc"), (v, "cfc"), (w, "ccf"))):
        A = np.array(geom.interior(np.asarray(U), loc), dtype=LD)
        topo, n = geom.topo[d], geom.N[d]
        df = geom.spacing(d)[1]
        if topo == "Periodic":
            A -= dt * (p - np.roll(p, 1, axis=d)) / _along(df[:n], d)
        elif topo == "Bounded":
            inner = tuple(slice(1, n) if q == d else slice(None) for q in range(3))
            up = tuple(slice(1, n) if q == d else slice(None) for q in range(3))
            dn = tuple(slice(0, n - 1) if q == d else slice(None) for q in range(3))
            A[inner] -= dt * (p[up] - p[dn]) / _along(df[1:n], d)
        out.append(A)
    return out


def condition_estimate(geom):
    """the project's estimate of the condition number of the discrete Laplacian on the unit box, the one of
    test_split_pressure_step_equals_library_plans: (4 Nx² + 4 Ny² + 4 / min Δz²) / (2π)²; a Flat direction contributes nothing"""
    terms = [4.0 * geom.N[0] ** 2 if geom.topo[0] != "Flat" else 0.0, 4.0 * geom.N[1] ** 2 if geom.topo[1] != "Flat" else 0.0,
             4.0 / float(geom.dzc.min()) ** 2 if geom.topo[2] != "Flat" else 0.0]
    return sum(terms) / (2 * np.pi) ** 2
