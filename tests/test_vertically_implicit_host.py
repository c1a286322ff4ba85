"""CPU tests that pin the numpy restatement of the vertically implicit ScalarDiffusivity (tests/vertically_implicit_reference.py) -- the
yardstick of tests/test_gpu_vertically_implicit.py -- and the Python surface of the feature:
  * the explicit part with the flag off is the oracle's closure term bit for bit; with the flag on it differs through the z fluxes at
    2 <= k <= Nz only;
  * the Thomas restatement solves the assembled matrix (dense numpy solve, tolerance from the matrix's own condition number), and the
    assembled rows are the second-difference operator on a regular grid;
  * the Python-orchestrated RK3 / AB2 step built from the oracle's exported pieces is the oracle's own time step bit for bit;
  * constructor forms, repr, refusals and exports."""
import numpy as np
import pytest

from helpers import smooth_state, tanh_faces
import vertically_implicit_reference as R

CASES = {
    "ppb_stretched": dict(size=(16, 16, 12), topo=(0, 0, 1), stretched=True),
    "bbb": dict(size=(12, 10, 8), topo=(1, 1, 1), stretched=False),
}


def _grid(O, name):
    c = CASES[name]
    z = tanh_faces(c["size"][2]) if c["stretched"] else (-1.0, 0.0)
    return O.Grid(c["size"], topology=c["topo"], x=(0.0, 1.0), y=(0.0, 1.0), z=z)


def _random_parents(g, seed, names=("u", "v", "w", "c")):
    """parent arrays of random interior values with the oracle's default halo fill"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in names:
        loc = R.LOCS[n]
        a = g.zeros(loc)
        g.interior(a, loc)[...] = rng.standard_normal(g.interior(a, loc).shape)
        g.fill_halo_regions(a, loc)
        out[n] = a
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_explicit_part_flag_off_is_the_oracle_closure_term(oracle, name):
    g = _grid(oracle, name)
    m = R.Metrics.of_oracle(g)
    P = _random_parents(g, 7)
    rng = np.random.default_rng(8)
    for f, which in enumerate("uvwc"):
        coef = 0.37 if which != "c" else 0.11
        G0 = g.zeros(R.LOCS[which])
        g.interior(G0, R.LOCS[which])[...] = rng.standard_normal(g.interior(G0, R.LOCS[which]).shape)
        G_ref = G0.copy(order="F")
        oracle.lib().oro_add_closure_tendency(g.handle, f, oracle._dp(P["u"]), oracle._dp(P["v"]), oracle._dp(P["w"]),
                                              oracle._dp(P["c"]) if which == "c" else None, coef, oracle._dp(G_ref), None)
        G_np = R.explicit_part(m, which, P, P["c"], coef, G0.copy(order="F"), vi=False)
        assert np.array_equal(G_np, G_ref), (which, np.abs(G_np - G_ref).max())
        assert not np.array_equal(G_ref, G0)


@pytest.mark.parametrize("name", list(CASES))
def test_explicit_part_flag_on_differs_through_the_interior_z_fluxes_only(oracle, name):
    """by construction: the z fluxes with the flag are the explicit ones at the flux indices 1 and Nz + 1 and the stated expressions at
    2 .. Nz, and the divergence assembled from the explicit x, y fluxes and these z fluxes is what explicit_part subtracts"""
    g = _grid(oracle, name)
    m = R.Metrics.of_oracle(g)
    P = _random_parents(g, 9)
    Nz = m.N[2]
    for which in "uvwc":
        coef = 0.37 if which != "c" else 0.11
        rng = m.default_range(R.LOCS[which], which != "c")
        W = R._Window(m, rng)
        on, off = R.z_fluxes(m, which, P, P["c"], coef, True, rng), R.z_fluxes(m, which, P, P["c"], coef, False, rng)
        edges = 0
        for side, dk in enumerate((0, -1) if which == "w" else (1, 0)):
            kk = np.broadcast_to(W.k(dk), on[side].shape)
            edge = (kk == 1) | (kk == Nz + 1)
            edges += int(edge.sum())
            assert (~edge).any()
            assert np.array_equal(on[side][edge], off[side][edge])
            if which == "u":
                inner = -(coef * W.ddx_f(P["w"], (0, 0, dk)))
            elif which == "v":
                inner = -(coef * W.ddy_f(P["w"], (0, 0, dk)))
            else:
                inner = np.zeros(on[side].shape)
            assert np.array_equal(on[side][~edge], inner[~edge])
            assert not np.array_equal(on[side][~edge], off[side][~edge])
        assert edges > 0                                 # (w's own range starts at face 2: only its lower flux meets the index 1)
        # the same assembly with either set of z fluxes: the x and y fluxes do not know the flag
        assert np.array_equal(R.closure_divergence(m, which, P, P["c"], coef, rng, vi=True),
                              R.closure_divergence(m, which, P, P["c"], coef, rng, vi=False, zflux=on))
        assert np.array_equal(R.closure_divergence(m, which, P, P["c"], coef, rng, vi=False),
                              R.closure_divergence(m, which, P, P["c"], coef, rng, vi=True, zflux=off))


def _metrics(size, topo, stretched):
    from oracle import oracle as O
    z = tanh_faces(size[2]) if stretched else (-1.0, 0.0)
    return R.Metrics.of_oracle(O.Grid(size, topology=topo, x=(0.0, 1.0), y=(0.0, 1.0), z=z))


def dense_tolerance(A, x):
    """bound on |Thomas - dense solve| in the max norm. Both are backward stable on these matrices (diagonal >= 1, non-positive
    off-diagonals, diagonally dominant by rows up to the reference's index shifts: no pivot growth), so each result is the exact solution
    of a system perturbed by a few eps |A| entrywise, and the two differ by at most 2 * (a few eps) * cond_inf(A) * |x|_inf -- the
    matrix's own condition number, 3 nonzeros per row, a factor 4 for the constants of the two backward-error bounds"""
    cond = np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf)
    return 2 * 4 * 3 * R.EPS * cond * np.abs(x).max()


@pytest.mark.parametrize("which", list("uvwc"))
@pytest.mark.parametrize("size,topo,stretched", [((5, 4, 13), (0, 0, 1), True), ((6, 5, 8), (1, 1, 1), False), ((3, 3, 2), (0, 0, 1), True)])
@pytest.mark.parametrize("r", [1.0, 100.0])
def test_thomas_restatement_solves_the_assembled_matrix(oracle, which, size, topo, stretched, r):
    m = _metrics(size, topo, stretched)
    loc = R.LOCS[which]
    dt = r * float(m.dzc.min()) ** 2 / 1.7               # the off-diagonals are O(r): Δt κ / Δz²
    a, b, c = R.diagonals(m, loc, 1.7, dt)
    off = max(np.abs(a[:, :, :-1]).max(), np.abs(c[:, :, :-1]).max())
    assert r / 8 < off <= 1.01 * r
    assert b.min() >= 1.0 and a.max() <= 0.0 and c.max() <= 0.0
    f = np.random.default_rng(3).standard_normal(size)
    phi = R.thomas(a, b, c, f.copy())
    for i in range(size[0]):
        for j in range(size[1]):
            A = R.dense_matrix(a, b, c, i, j)
            x = np.linalg.solve(A, f[i, j, :])
            assert np.abs(phi[i, j, :] - x).max() <= dense_tolerance(A, x), (i, j)
    if topo[0] == 1 and which == "u":                    # the wall-face column of u: every off-diagonal zeroed, the identity
        assert np.array_equal(phi[0], f[0]) and not np.array_equal(phi[1], f[1])
        assert np.all(a[0] == 0) and np.all(c[0] == 0) and np.all(b[0] == 1)
    if topo[1] == 1 and which == "v":
        assert np.array_equal(phi[:, 0], f[:, 0]) and np.all(b[:, 0] == 1)


@pytest.mark.parametrize("which", list("uvwc"))
def test_assembled_rows_are_the_second_difference_operator_on_a_regular_grid(oracle, which):
    """on a regular grid the reference's index shifts cannot matter: row k is 1 + Δt κ (n_k / Δz²) on the diagonal and -Δt κ / Δz² beside
    it, n_k the number of neighbours the row couples to. Center fields: no-flux rows at k = 1 and Nz. w: rows 1 .. Nz of the faces, the
    wall face k = 1 coupled upwards only (not an identity row), face Nz coupled to both sides (face Nz + 1 is outside the system)."""
    Nz, kappa, dt = 8, 0.3, 0.05
    m = _metrics((4, 3, Nz), (0, 0, 1), False)
    a, b, c = R.diagonals(m, R.LOCS[which], kappa, dt)
    dz = 1.0 / Nz
    r = dt * kappa / dz ** 2
    A = R.dense_matrix(a, b, c, 1, 1)
    E = np.zeros((Nz, Nz))
    for k in range(Nz):
        lo, hi = k > 0, k < Nz - 1
        if lo:
            E[k, k - 1] = -r
        if hi:
            E[k, k + 1] = -r
        n = (lo + hi) if which != "w" else (lo + 1)      # w: the upper coefficient is never zeroed (peripheral_node at the Center k)
        E[k, k] = 1 + n * r
    assert np.allclose(A, E, rtol=8 * R.EPS, atol=0)
    if which == "w":
        assert A[0, 0] != 1.0 and A[0, 1] != 0.0


BCS = {"c0": {"top": ("value", 0.4)}, "c1": {"bottom": ("flux", 0.03)}}


def _smooth_values(g, seed):
    """helpers.smooth_state on the nodes of an oracle grid, under the oracle's field names"""
    locs = {"u": R.LOCS["u"], "v": R.LOCS["v"], "w": R.LOCS["w"], "T": R.LOCS["c"], "S": R.LOCS["c"]}

    def nodes(loc):
        out = []
        for d in range(3):
            n = g.N[d] + (1 if (loc[d] == 1 and g.topo[d] == 1) else 0)
            x = (0.0, 0.0, -1.0)[d] + (np.arange(n) + (0.0 if loc[d] == 1 else 0.5)) / g.N[d]
            out.append(x.reshape([-1 if q == d else 1 for q in range(3)]))
        return tuple(out)

    vals = smooth_state({n: nodes(l) for n, l in locs.items()}, seed)
    vals["c0"], vals["c1"] = vals.pop("T"), vals.pop("S")
    return vals


@pytest.mark.parametrize("stepper", ["rk3", "ab2"])
@pytest.mark.parametrize("name", list(CASES))
def test_orchestrated_step_is_the_oracle_time_step(oracle, name, stepper):
    """the orchestration is pinned: with the oracle's explicit closure term it reproduces oro_model_time_step bit for bit (u, v, w,
    tracers, p, clock) over 2 steps; with the numpy explicit part (flag off) as well"""
    g = _grid(oracle, name)
    nu, kappa = 2e-3, (5e-3, 1e-3)
    vals = _smooth_values(g, 11)
    ref = oracle.Model(g, 2)
    ref.set_closure(nu, kappa)
    for n, sides in BCS.items():
        for side, (kind, value) in sides.items():
            ref.set_bc(n, side, kind, value)
    ref.set(**vals)
    dt = 0.05 / g.N[0]
    models = [R.Orchestrated(oracle, g, 2, nu, kappa, closure=how, bcs=BCS) for how in ("oracle", "numpy")]
    for o in models:
        o.set(**vals)
    for _ in range(2):
        ref.time_step(dt) if stepper == "rk3" else ref.time_step_ab2(dt)
        for o in models:
            o.time_step(dt) if stepper == "rk3" else o.time_step_ab2(dt)
    for o in models:
        for n in o.names:
            assert np.array_equal(o.U[n], ref.field(n)), (o.closure, n)
        assert np.array_equal(o.p, ref.field("p")), o.closure
        assert o.time == ref.time and o.iteration == ref.iteration == 2
    assert np.abs(ref.field("c1")).max() > 0


def test_orchestrated_vertically_implicit_step_differs_and_stays_bounded(oracle):
    """the yardstick itself: the same script with the numpy explicit part (flag on) and the numpy solve is another scheme (it differs
    from the explicit one) of the same equations (by O(Δt) only)"""
    g = _grid(oracle, "ppb_stretched")
    vals = _smooth_values(g, 11)
    dt = 0.05 / g.N[0]
    out = {}
    for how in ("numpy", "vi"):
        o = R.Orchestrated(oracle, g, 2, 2e-3, (5e-3, 1e-3), closure=how, bcs=BCS)
        o.set(**vals)
        o.time_step(dt)
        out[how] = o
    for n in out["vi"].names:
        a, b = out["vi"].U[n], out["numpy"].U[n]
        assert np.all(np.isfinite(a)) and not np.array_equal(a, b)
        assert np.abs(a - b).max() < 1e-2 * max(np.abs(b).max(), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_constructor_forms_and_repr():
    import oldoceananigans_jl_amd as ocn
    VI, EX = ocn.VerticallyImplicitTimeDiscretization, ocn.ExplicitTimeDiscretization
    c = ocn.ScalarDiffusivity(VI(), ν=1e-2, κ=2e-3)
    assert isinstance(c.time_discretization, VI) and (c.ν, c.κ) == (1e-2, 2e-3)
    assert repr(c) == "ScalarDiffusivity{VerticallyImplicitTimeDiscretization}(ν=0.01, κ=0.002)"
    c = ocn.ScalarDiffusivity(ν=1e-2, κ={"T": 1e-3, "S": 2e-3}, time_discretization=VI())
    assert isinstance(c.time_discretization, VI) and c.κ == {"T": 1e-3, "S": 2e-3}
    c = ocn.ScalarDiffusivity(VI(), 1e-2, 2e-3)
    assert isinstance(c.time_discretization, VI) and (c.ν, c.κ) == (1e-2, 2e-3)
    # a number in first position keeps meaning ν, exactly as before
    c = ocn.ScalarDiffusivity(1e-2, 2e-3)
    assert type(c.time_discretization) is EX and (c.ν, c.κ) == (1e-2, 2e-3)
    assert repr(c) == "ScalarDiffusivity{ExplicitTimeDiscretization}(ν=0.01, κ=0.002)"
    assert repr(ocn.ScalarDiffusivity(ν=1.0)) == "ScalarDiffusivity{ExplicitTimeDiscretization}(ν=1.0, κ=0.0)"
    assert type(ocn.ScalarDiffusivity(EX(), ν=1.0).time_discretization) is EX
    assert ocn.ScalarDiffusivity(nu=3.0, kappa=4.0).κ == 4.0
    with pytest.raises(TypeError):
        ocn.ScalarDiffusivity(VI(), ν=1.0, time_discretization=VI())
    with pytest.raises(TypeError):
        ocn.ScalarDiffusivity(ν=1.0, time_discretization="implicit")
    with pytest.raises(ValueError):
        ocn.ScalarDiffusivity(VI(), ν=-1.0)


def test_refusals():
    import oldoceananigans_jl_amd as ocn
    VI = ocn.VerticallyImplicitTimeDiscretization
    for make in (lambda: ocn.AnisotropicMinimumDissipation(VI()), lambda: ocn.AnisotropicMinimumDissipation(time_discretization=VI()),
                 lambda: ocn.Smagorinsky(VI()), lambda: ocn.Smagorinsky(time_discretization=VI()), lambda: ocn.SmagorinskyLilly(VI()),
                 lambda: ocn.SmagorinskyLilly(time_discretization=VI())):
        with pytest.raises(NotImplementedError, match="VerticallyImplicitTimeDiscretization"):
            make()
    with pytest.raises(NotImplementedError, match="VerticalScalarDiffusivity"):
        ocn.VerticalScalarDiffusivity(VI(), ν=1.0)
    # the explicit discretisation of the eddy-coefficient closures is what it was
    assert ocn.Smagorinsky(ocn.ExplicitTimeDiscretization()).coefficient == 0.16
    assert ocn.AnisotropicMinimumDissipation(ocn.ExplicitTimeDiscretization()).Cν == 1 / 3
    assert ocn.SmagorinskyLilly(0.2, 0.5).coefficient == 0.2
    # a Periodic z is the reference's error (vertically_implicit_diffusion_solver.jl:149-153), raised before anything touches the device
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    with pytest.raises(ValueError, match="Bounded in the z-direction"):
        ocn.NonhydrostaticModel(grid=grid, closure=ocn.ScalarDiffusivity(VI(), ν=1e-3))


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ocn_mi355x.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _lib.lib()
    for s in ("ocn_compute_closure_tendencies_vertically_implicit", "ocn_implicit_step_z", "ocn_model_set_vertically_implicit"):
        assert s + "(" in header and s in _lib.SYMBOLS and hasattr(lib, s)
        assert f"(:{s}, libocn)" in integration
    for n in ("VerticallyImplicitTimeDiscretization", "ExplicitTimeDiscretization", "VerticalScalarDiffusivity"):
        assert n in ocn.__all__
    assert callable(ocn.kernels.implicit_step) and callable(ocn.kernels.compute_closure_tendencies_vertically_implicit)
