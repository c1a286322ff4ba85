"""CPU tests of tilted domains (BuoyancyForce(gravity_unit_vector), ConstantCartesianCoriolis): the constructors against numbers the
reference holds (docs/src/model_setup/coriolis.md:48-70, test/test_coriolis.jl:28-38,109-113, the BuoyancyForce docstring), and the numpy
restatement (tests/tilted_reference.py) pinned independently of the kernels -- to the oracle where the two overlap, and to the analytic
f × U where every product is exact."""
import math

import numpy as np
import pytest

import tilted_reference as T
import vertically_implicit_reference as R
from helpers import smooth_state, tanh_faces

EPS = R.EPS


# ---------------------------------------------------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------------------------------------------------
def _approx(a, b):
    """Julia's isapprox: rtol = √eps"""
    return abs(a - b) <= math.sqrt(EPS) * max(abs(a), abs(b))


def test_constant_cartesian_coriolis_of_the_documentation():
    """docs/src/model_setup/coriolis.md:48-70: three spellings of f = (0, 2, 1) x 1e-4, and latitude 45 on Earth"""
    import oldoceananigans_jl_amd as ocn
    want = "ConstantCartesianCoriolis{Float64}: fx = 0.00e+00, fy = 2.00e-04, fz = 1.00e-04"
    a = ocn.ConstantCartesianCoriolis(fx=0, fy=2e-4, fz=1e-4)
    norm = math.sqrt(2e-4 ** 2 + 1e-4 ** 2)
    axis = tuple(c / norm for c in (0, 2e-4, 1e-4))
    assert axis == (0.0, 0.8944271909999159, 0.4472135954999579)                  # the doctest's printed axis
    b = ocn.ConstantCartesianCoriolis(f=norm, rotation_axis=axis)
    for c in (a, b):
        assert c.fx == 0 and _approx(c.fy, 2e-4) and _approx(c.fz, 1e-4) and repr(c) == want
    assert (a.fx, a.fy, a.fz) == (0.0, 2e-4, 1e-4)
    lat = ocn.ConstantCartesianCoriolis(rotation_rate=7.292115e-5, latitude=45)
    assert repr(lat) == "ConstantCartesianCoriolis{Float64}: fx = 0.00e+00, fy = 1.03e-04, fz = 1.03e-04"
    assert lat.fx == 0 and lat.fy == 2 * 7.292115e-5 * 0.7071067811865476 == lat.fz           # cosd(45) == sind(45) in Julia
    # the default rotation axis is ZDirection(): an f-plane
    z = ocn.ConstantCartesianCoriolis(f=1e-4)
    assert (z.fx, z.fy, z.fz) == (0.0, 0.0, 1e-4)
    assert (ocn.ConstantCartesianCoriolis(f=1e-4, rotation_axis=ocn.ZDirection()).fz) == 1e-4


def test_constant_cartesian_coriolis_of_the_reference_tests():
    """test/test_coriolis.jl:28-38 (values) and :109-113 (the four throwing calls; ArgumentError -> ValueError)"""
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd.buoyancy import cosd, sind
    assert cosd(45) == sind(45) == 0.7071067811865476 and cosd(60) == 0.5 and cosd(90) == 0.0 and cosd(0) == 1.0 and cosd(180) == -1.0
    c = ocn.ConstantCartesianCoriolis(f=1, rotation_axis=[0, cosd(45), sind(45)])
    assert _approx(c.fy, cosd(45)) and _approx(c.fz, sind(45)) and c.fx == 0
    t = math.sqrt(1 / 3)
    c = ocn.ConstantCartesianCoriolis(f=10, rotation_axis=[t, t, t])
    assert _approx(c.fx, 10 * t) and _approx(c.fy, 10 * t) and _approx(c.fz, 10 * t)
    for kw in (dict(rotation_axis=[0, 1, 1]), dict(f=1, latitude=45), dict(fx=1, latitude=45), dict(fx=1, f=1)):
        with pytest.raises(ValueError):
            ocn.ConstantCartesianCoriolis(**kw)
    with pytest.raises(ValueError, match="unit vector"):
        ocn.ConstantCartesianCoriolis(f=1, rotation_axis=[0, 1, 1])                # a rotation axis that is no unit vector


def test_buoyancy_force_and_unit_vectors():
    """the summary of the BuoyancyForce docstring (buoyancy_force.jl:28-43) and validate_unit_vector (Grids/input_validation.jl:174-186)"""
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd.buoyancy import cosd, sind
    θ = 45
    bf = ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0, -sind(θ), -cosd(θ)))
    assert repr(bf) == "BuoyancyTracer with ĝ = (0.0, -0.707107, -0.707107)"
    assert bf.required_tracers == ("b",) and bf.tilted and bf.gravity_unit_vector == (0.0, -sind(θ), -cosd(θ))
    sw = ocn.BuoyancyForce(ocn.SeawaterBuoyancy())
    assert sw.required_tracers == ("T", "S") and not sw.tilted and isinstance(sw.gravity_unit_vector, ocn.NegativeZDirection)
    assert repr(sw) == "SeawaterBuoyancy with ĝ = NegativeZDirection()"
    v = ocn.validate_unit_vector
    assert isinstance(v(ocn.ZDirection()), ocn.ZDirection) and isinstance(v(ocn.NegativeZDirection()), ocn.NegativeZDirection)
    assert v([0, 0.6, 0.8]) == (0.0, 0.6, 0.8) and v(np.array([1.0, 0.0, 0.0])) == (1.0, 0.0, 0.0)
    assert v((0, 0, 1 + 1e-9)) == (0.0, 0.0, 1 + 1e-9)                              # inside rtol = √eps ~ 1.5e-8 of the squared norm
    with pytest.raises(ValueError, match="length 3"):
        v((0, 1))
    with pytest.raises(ValueError, match="≈ 1"):
        v((0, 0, 1 + 1e-7))
    with pytest.raises(ValueError, match="≈ 1"):
        v((0, 1, 1))
    for name in ("BuoyancyForce", "ConstantCartesianCoriolis", "ZDirection", "NegativeZDirection", "validate_unit_vector"):
        assert name in ocn.__all__, name


def test_refusals_before_any_handle():
    """a non-unit gravity vector; a partitioned grid (refused on grid metadata: this runs without a GPU)"""
    import oldoceananigans_jl_amd as ocn
    with pytest.raises(ValueError, match="≈ 1"):
        ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0, 1, -1))
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))

    class Partitioned:                                     # what DistributedRectilinearGrid looks like to the model: a `local` grid
        local = grid
        halo_size = grid.halo_size
    tilted = ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0.6, 0, -0.8))
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=Partitioned(), tracers=("b",), buoyancy=tilted)
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=Partitioned(), tracers=(), coriolis=ocn.ConstantCartesianCoriolis(fx=0, fy=1, fz=1))
    with pytest.raises(NotImplementedError, match="coriolis must be"):
        ocn.NonhydrostaticModel(grid=grid, coriolis="BetaPlane")
    with pytest.raises(NotImplementedError, match="buoyancy must be"):
        ocn.NonhydrostaticModel(grid=grid, buoyancy=ocn.BuoyancyForce("TEOS10"))


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import oldoceananigans_jl_amd as ocn
    from oldoceananigans_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ocn_mi355x.h")).read()
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    lib = _lib.lib()
    for s in ("ocn_add_cartesian_coriolis", "ocn_add_buoyancy_acceleration", "ocn_update_hydrostatic_pressure_tilted",
              "ocn_model_set_cartesian_coriolis", "ocn_model_set_gravity_unit_vector"):
        assert s + "(" in header and s in _lib.SYMBOLS and hasattr(lib, s)
        assert f"(:{s}, libocn)" in integration
    for key in ("coriolis_kind", "tilted_gravity"):
        assert key in header
    for fn in ("add_cartesian_coriolis", "add_buoyancy_acceleration", "update_hydrostatic_pressure_tilted"):
        assert callable(getattr(ocn.kernels, fn))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, pinned independently of the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
def test_hydrostatic_recurrence_with_vertical_gravity_is_the_oracle(oracle, kind):
    """ĝ = (0, 0, 1): the restated recurrence == oro_update_hydrostatic_pressure on a tanh-stretched 6 x 5 x 9 grid, both buoyancy kinds"""
    O = oracle
    g = O.Grid((6, 5, 9), topology=(0, 0, 1), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(9))
    m = R.Metrics.of_oracle(g)
    r = np.random.default_rng(2)
    bT = np.asfortranarray(r.standard_normal(g.parent_size(R.LOCS["c"])))
    S = np.asfortranarray(35 + r.standard_normal(bT.shape))
    grav, alpha, beta = 9.80665, 1.67e-4, 7.8e-4
    fill = 7.0                                            # entries outside i = 0:Nx+1, j = 0:Ny+1, k = 1:Nz keep their values
    want = np.full(bT.shape, fill, order="F")
    O.lib().oro_update_hydrostatic_pressure(g.handle, kind, O._dp(bT), O._dp(S) if kind == 2 else None, grav, alpha, beta, O._dp(want))
    got = np.full(bT.shape, fill, order="F")
    T.hydrostatic_pressure(m, 1.0, T.buoyancy_perturbation(kind, bT, S, grav, alpha, beta), got)
    assert np.array_equal(got, want) and np.count_nonzero(got != fill) == 8 * 7 * 9
    # ĝ_z = 0.5: exactly half (a power of two scales every operation of the recurrence exactly)
    half = np.full(bT.shape, fill, order="F")
    T.hydrostatic_pressure(m, 0.5, T.buoyancy_perturbation(kind, bT, S, grav, alpha, beta), half)
    inside = got != fill
    assert np.array_equal(half[inside], 0.5 * got[inside])


def test_uniform_fields_give_the_exact_cross_product(oracle):
    """U = (2, -0.5, 4), f = (0.25, -2, 0.5) on a triply periodic 6 x 5 x 4 grid: every product and sum is exact, so the three components ==
    the analytic f × U at every point; with b ≡ 1, x_dot_g_b == -gravity_unit_vector[0] and y_dot_g_b == -gravity_unit_vector[1]. This
    pins the signs on something the kernels and the restatement do not share."""
    g = oracle.Grid((6, 5, 4), topology=(0, 0, 0), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
    m = R.Metrics.of_oracle(g)
    Uv, f = (2.0, -0.5, 4.0), (0.25, -2.0, 0.5)
    U = {n: np.full(g.parent_size(R.LOCS[n]), val, order="F") for n, val in zip("uvw", Uv)}
    cross = (f[1] * Uv[2] - f[2] * Uv[1], f[2] * Uv[0] - f[0] * Uv[2], f[0] * Uv[1] - f[1] * Uv[0])
    assert cross == (-7.75, 0.0, 3.875)
    rng = (1, 6, 1, 5, 1, 4)
    for term, want in zip((T.x_f_cross_U, T.y_f_cross_U, T.z_f_cross_U), cross):
        got = term(m, f, U, rng)
        assert got.shape == (6, 5, 4) and np.all(got == want), (term.__name__, want)
    # f × U with a nonzero y component as well
    f2 = (0.25, -2.0, 1.5)
    assert np.all(T.y_f_cross_U(m, f2, U, rng) == f2[2] * Uv[0] - f2[0] * Uv[2]) and f2[2] * Uv[0] - f2[0] * Uv[2] == 2.0
    G = {n: np.zeros(g.parent_size(R.LOCS[n]), order="F") for n in "uvw"}
    T.add_cartesian_coriolis(m, f2, U, G)
    for n, want in zip("uvw", (f2[1] * Uv[2] - f2[2] * Uv[1], 2.0, 3.875)):
        assert np.all(g.interior(G[n], R.LOCS[n]) == -want), n                       # G -= f × U
    gravity_unit_vector = (0.6, 0.0, -0.8)
    ghat = tuple(-c for c in gravity_unit_vector)
    b = np.ones(g.parent_size(R.LOCS["c"]), order="F")
    assert np.all(T.x_dot_g_b(m, ghat[0], b, rng) == -gravity_unit_vector[0])
    assert np.all(T.y_dot_g_b(m, ghat[1], b, rng) == -gravity_unit_vector[1])
    assert np.all(T.x_dot_g_b(m, 0.25, b, rng) == 0.25) and np.all(T.y_dot_g_b(m, -0.5, 3 * b, rng) == -1.5)
    G = {n: np.zeros(g.parent_size(R.LOCS[n]), order="F") for n in "uv"}
    T.add_buoyancy_acceleration(m, (0.25, -0.5, 0.0), b, G)
    assert np.all(g.interior(G["u"], R.LOCS["u"]) == 0.25) and np.all(g.interior(G["v"], R.LOCS["v"]) == -0.5)     # G += ĝ b


def test_vertical_rotation_vector_agrees_with_the_fplane_of_the_oracle(oracle):
    """f = (0, 0, f) on a triply periodic grid, smooth state: against oro_add_fplane_coriolis. Not `==`: with every node active FPlane forms
    f * ½(½(v₁ + v₂) + ½(v₃ + v₄)) -- x pairs first, one product -- and ConstantCartesianCoriolis ½(f ½(v₁ + v₃) + f ½(v₂ + v₄)) -- y
    pairs first, the product inside. Halvings are exact; each form rounds three times on the way (pair sum, outer sum, product -- in
    either order), each by at most u = ε/2 relative, on magnitudes of at most |f| max|v|: each form lies within ((1 + u)³ - 1) |f| max|v| of
    the exact value, the two within 6u (1 + 2u) |f| max|v| < 3ε (1 + 4ε) |f| max|v| of each other. The w tendency is unchanged."""
    O = oracle
    g = O.Grid((8, 6, 4), topology=(0, 0, 0), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
    m = R.Metrics.of_oracle(g)
    nodes = {}
    for n in "uvw":
        idx = [np.arange(s, dtype=np.float64) for s in g.parent_size(R.LOCS[n])]
        nodes[n] = (idx[0][:, None, None] / 8, idx[1][None, :, None] / 6, idx[2][None, None, :] / 4)
    vals = smooth_state(nodes, 8)
    U = {n: np.asfortranarray(vals[n]) for n in "uvw"}
    for n in "uvw":
        g.fill_halo_regions(U[n], R.LOCS[n])
    f = 0.7
    r = np.random.default_rng(6)
    G0 = {n: np.asfortranarray(r.standard_normal(U[n].shape)) for n in "uvw"}
    want = {n: G0[n].copy(order="F") for n in "uvw"}
    O.lib().oro_add_fplane_coriolis(g.handle, f, O._dp(U["u"]), O._dp(U["v"]), O._dp(want["u"]), O._dp(want["v"]))
    got = T.add_cartesian_coriolis(m, (0.0, 0.0, f), U, {n: G0[n].copy(order="F") for n in "uvw"})
    assert np.array_equal(got["w"], G0["w"])
    for n, other in (("u", "v"), ("v", "u")):
        term = np.abs(g.interior(want[n], R.LOCS[n]) - g.interior(G0[n], R.LOCS[n])).max()
        bound = 3 * EPS * (1 + 4 * EPS) * abs(f) * np.abs(U[other]).max()
        # the tendencies hold G0 - term: the subtraction rounds once more on each side, by at most u |G| each
        bound += EPS * np.abs(want[n]).max()
        diff = np.abs(got[n] - want[n]).max()
        print(f"G{n}: max |cartesian - fplane| {diff:.3e}, bound {bound:.3e}, the term itself {term:.3e}")
        assert term > 0.1 and diff <= bound
        # the terms themselves, without the tendency's rounding
        rng = (1, 8, 1, 6, 1, 4)
        mine = (T.x_f_cross_U if n == "u" else T.y_f_cross_U)(m, (0.0, 0.0, f), U, rng)
        zero = {k: np.zeros_like(v) for k, v in G0.items()}
        O.lib().oro_add_fplane_coriolis(g.handle, f, O._dp(U["u"]), O._dp(U["v"]), O._dp(zero["u"]), O._dp(zero["v"]))
        theirs = -g.interior(zero[n], R.LOCS[n])              # 0 - term is exact
        assert np.abs(mine - theirs).max() <= 3 * EPS * (1 + 4 * EPS) * abs(f) * np.abs(U[other]).max()


def test_orchestrated_yardstick_without_the_new_terms_is_the_oracle_model(oracle):
    """TiltedOrchestrated with no rotation vector and NegativeZDirection() is the oracle's own model (BuoyancyTracer, FPlane,
    ScalarDiffusivity): two RK3 steps, =="""
    O = oracle
    g = O.Grid((8, 8, 8), topology=(0, 0, 1), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(8))
    nu, kappa = 2e-3, (5e-3,)
    mo = O.Model(g, 1)
    mo.set_closure(nu=nu, kappa=kappa)
    L = O.lib()
    L.oro_model_set_buoyancy(mo.handle, 1, 0, 0, 0.0, 0.0, 0.0)
    L.oro_model_set_coriolis.argtypes = [L.oro_model_set_buoyancy.argtypes[0], L.oro_model_set_buoyancy.argtypes[1], L.oro_add_fplane_coriolis.argtypes[1]]
    L.oro_model_set_coriolis(mo.handle, 1, 0.7)
    yard = T.TiltedOrchestrated(O, g, 1, nu, kappa, buoyancy_index=0, fcor=0.7, closure="oracle")
    r = np.random.default_rng(11)
    names = ["u", "v", "w", "c0"]
    vals = {n: 0.3 * r.standard_normal(g.interior(g.zeros(R.LOCS.get(n, R.LOCS["c"])), R.LOCS.get(n, R.LOCS["c"])).shape) for n in names}
    mo.set(**vals)
    yard.set(**vals)
    for _ in range(2):
        mo.time_step(0.01)
        yard.time_step(0.01)
    for n in names:
        assert np.all(np.isfinite(yard.U[n])) and np.array_equal(yard.U[n], mo.field(n)), n
    assert np.array_equal(yard.p, mo.field("p")) and yard.time == mo.time
