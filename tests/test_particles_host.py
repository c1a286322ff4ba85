"""CPU tests of Lagrangian particle tracking: the numpy restatement (tests/particles_reference.py) pinned by facts that do not depend on it,
the descriptor LagrangianParticles, and the bounds requirement of the device code on the host build of its index function
(ocn_particle_indices_host). No device is touched."""
import ctypes as C

import numpy as np
import pytest

import particles_reference as P

EPS = 2.220446049250313e-16
STRETCHED = [-1, -0.5, 0, 0.4, 0.7, 1]          # test_lagrangian_particle_tracking.jl:318


@pytest.fixture(scope="module")
def ocn():
    import oldoceananigans_jl_amd as ocn
    return ocn


def _grid(ocn, stretched, topo=("Periodic", "Periodic", "Bounded"), size=(5, 5, 5)):
    """the grids of test_lagrangian_particle_tracking.jl:305-326: x, y in (-1, 1), z in (-1, 1) or the stretched faces"""
    topology = tuple(getattr(ocn, t) for t in topo)
    kw = {d: (-1.0, 1.0) for d, t in zip("xy", topo) if t != "Flat"}
    return ocn.RectilinearGrid(None, size=size, topology=topology, z=STRETCHED if stretched else (-1.0, 1.0), **kw)


def _sample(grid, loc_classes, f):
    """the parent array of f(x, y, z) at the nodes of a location, halos included (the nodes continue linearly into the halo)"""
    ocn_loc = loc_classes
    shape = grid.total_size(ocn_loc)
    H = grid.halo_size
    import oldoceananigans_jl_amd as ocn
    coords = []
    for d, (F, Cn) in enumerate(((grid.xᶠᵃᵃ, grid.xᶜᵃᵃ), (grid.yᵃᶠᵃ, grid.yᵃᶜᵃ), (grid.zᵃᵃᶠ, grid.zᵃᵃᶜ))):
        a = np.asarray(F if ocn_loc[d] is ocn.Face else Cn, dtype=np.float64)
        if grid.topology[d] is ocn.Flat:
            a = a[:1]
        assert len(a) >= shape[d]
        coords.append(a[:shape[d]])
    X, Y, Z = np.meshgrid(*coords, indexing="ij")
    return np.asfortranarray(f(X, Y, Z)), coords


LOCS = {"ccc": (0, 0, 0), "fcc": (1, 0, 0), "cfc": (0, 1, 0), "ccf": (0, 0, 1)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. + 2. linear exactness; a node returns its value
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("loc", list(LOCS))
def test_linear_fields_interpolate_exactly(ocn, stretched, loc):
    """a + b x + c y + d z sampled at its own nodes, at 200 random points of the domain. Bound: the eight weights are non-negative and sum to
    1 within rounding, each is two products of (1 - ξ)-like factors (<= 5 roundings), each term one more product, the sum seven additions:
    <= 13 eps F with F = max |field|. The fractional index of direction d carries <= 3 roundings of size eps (N_d + 2) plus the distance of
    the Julia-range nodes from x₀ + (i - 1) Δ, <= 2 eps max|x| / Δ_d index units (for the stretched z: the four operations of
    fractional_index, the same count); an index error δ moves the value by δ |slope_d| Δ_d. The sum of both is the tolerance."""
    grid = _grid(ocn, stretched)
    g = P.Geometry.of_grid(grid)
    a, b, c, d = 0.3, 1.7, -0.8, 2.1
    classes = tuple(ocn.Face if l else ocn.Center for l in LOCS[loc])
    data, _ = _sample(grid, classes, lambda x, y, z: a + b * x + c * y + d * z)
    rng = np.random.default_rng(5)
    x, y, z = (rng.uniform(-1, 1, 200) for _ in range(3))
    got = P.interpolate(g, data, LOCS[loc], x, y, z)
    want = a + b * x + c * y + d * z
    F = np.abs(data).max()
    dmin_z = np.diff(STRETCHED).min() if stretched else g.d[2]
    bound = EPS * (13 * F + sum((3 * (N + 2) + 2 * 1.0 / dl) * abs(s) * dh
                                for N, dl, dh, s in ((5, g.d[0], g.d[0], b), (5, g.d[1], g.d[1], c), (5, dmin_z, 0.5 if stretched else g.d[2], d))))
    err = np.abs(got - want).max()
    print(f"{loc} stretched={stretched}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("loc", list(LOCS))
def test_a_node_returns_its_value(ocn, stretched, loc):
    """at a node ξ = η = ζ = 0: seven weights are 0, one is 1, and 0 * finite + value is the value, bit for bit. That needs the node's
    fractional index to be an exact integer, which the reference's arithmetic gives where (x - x₀) / Δ is exact: a regular direction with a
    dyadic spacing (8 cells on (-1, 1)), and every node of the stretched z but the last centre, which the search reaches as x₂ of the end
    pair, where 1 / (x₂ - x₁) * (x₂ - x₁) need not be 1."""
    grid = _grid(ocn, stretched, size=(8, 8, 5 if stretched else 8))
    g = P.Geometry.of_grid(grid)
    classes = tuple(ocn.Face if l else ocn.Center for l in LOCS[loc])
    rng = np.random.default_rng(2)
    data, coords = _sample(grid, classes, lambda x, y, z: rng.standard_normal(x.shape))
    H = grid.halo_size
    I, J, K = np.meshgrid(np.arange(1, 9), np.arange(1, 9), np.arange(1, 5 if stretched else 9), indexing="ij")
    I, J, K = I.ravel(), J.ravel(), K.ravel()
    x, y, z = coords[0][I - 1 + H[0]], coords[1][J - 1 + H[1]], coords[2][K - 1 + H[2]]
    (i0, _, xi), (j0, _, eta), (k0, _, zeta) = P.interpolators(g, LOCS[loc], x, y, z)
    assert np.array_equal(i0, I) and np.array_equal(j0, J) and np.array_equal(k0, K)
    assert not xi.any() and not eta.any() and not zeta.any()
    got = P.interpolate(g, data, LOCS[loc], x, y, z)
    assert np.array_equal(got, data[I - 1 + H[0], J - 1 + H[1], K - 1 + H[2]])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the reference's restitution test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretched", [False, True])
@pytest.mark.parametrize("topo,size", [(("Periodic", "Periodic", "Bounded"), (5, 5, 5)), (("Periodic", "Flat", "Bounded"), (5, 5))])
def test_reference_restitution_case(ocn, stretched, topo, size):
    """test_lagrangian_particle_tracking.jl:84-104: a particle at z_c[Nz - 1] between w[Nz - 1] and w[Nz] gets w = (0.15 + top - z₀) / Δt,
    leaves through the top by 0.15 and bounces back (Cʳ = 1) to top - 0.15; ≈ is rtol = √eps"""
    grid = _grid(ocn, stretched, topo, size)
    g = P.Geometry.of_grid(grid)
    Nz, Hz = grid.Nz, grid.Hz
    top = float(grid.zᵃᵃᶠ[Nz + Hz])
    z0 = float(grid.zᵃᵃᶜ[Nz - 2 + Hz])
    dt = 0.01
    shape = lambda loc: grid.total_size(loc)                                                # noqa: E731
    u = np.zeros(shape((ocn.Face, ocn.Center, ocn.Center)), order="F")
    v = np.zeros(shape((ocn.Center, ocn.Face, ocn.Center)), order="F")
    w = np.zeros(shape((ocn.Center, ocn.Center, ocn.Face)), order="F")
    w[:, :, Nz - 1 + Hz] = (0.1 + top - z0) / dt
    w[:, :, Nz - 2 + Hz] = (0.2 + top - z0) / dt
    x, y, z = P.advect(g, [0.0], [0.0], [z0], u, v, w, dt, 1.0)
    assert x[0] == 0.0 and y[0] == 0.0
    assert abs(z[0] - (top - 0.15)) <= np.sqrt(EPS) * max(abs(z[0]), abs(top - 0.15))


# ---------------------------------------------------------------------------------------------------------------------
# 4. boundary rules by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_boundary_rules_by_hand():
    xL, xR = -1.0, 3.0                                   # length 4: every value below is exact in binary
    per = lambda x: float(P.enforce(P.PERIODIC, x, xL, xR, 1.0))                            # noqa: E731
    assert per(3.5) == -0.5 and per(-1.5) == 2.5 and per(0.25) == 0.25
    assert per(3.0) == 3.0 and per(-1.0) == -1.0                   # on a face: inside, unchanged
    assert per(3.0 + 9.5) == -1.0 + 1.5 and per(-1.0 - 9.5) == 3.0 - 1.5          # more than two domain lengths
    assert per(7.0) == -1.0 and per(-5.0) == 3.0                   # a whole length: mod = 0, lands on the near wall
    bnc = lambda x, Cr: float(P.enforce(P.BOUNDED, x, xL, xR, Cr))                          # noqa: E731
    assert bnc(3.5, 1.0) == 2.5 and bnc(3.5, 0.5) == 2.75 and bnc(3.5, 0.0) == 3.0
    assert bnc(-2.0, 1.0) == 0.0 and bnc(-2.0, 0.5) == -0.5 and bnc(-2.0, 0.0) == -1.0
    assert bnc(1.0, 0.5) == 1.0
    assert bnc(3.0 + 5.0, 1.0) == -1.0 and bnc(-1.0 - 5.0, 1.0) == 3.0            # the bounce would leave through the far wall: clamped
    assert bnc(3.0 + 5.0, 0.5) == 0.5
    assert float(P.enforce(P.FLAT, 17.0, 0.0, 1.0, 1.0)) == 17.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. index edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_index_edge_cases():
    # trunc towards zero against the floored mod: they disagree for a negative fractional index, on purpose
    im, ip, xi = P.interpolator(np.array([-0.3, 0.7, 2.0, -1.0, -1.25]))
    assert im.tolist() == [0, 0, 2, -1, -1] and ip.tolist() == [1, 1, 3, 0, 0]
    assert xi[0] == P.julia_mod(-0.3, 1.0) == 1.0 - 0.3 and xi[1] == 0.7 and xi[2] == 0.0 and xi[3] == 0.0 and xi[4] == 0.75
    assert not np.signbit(P.julia_mod(-2.0, 1.0))        # +0.0, the sign of the divisor
    vec = np.array(STRETCHED, dtype=np.float64)
    # an exact node returns (mid + 1, mid + 1) where the search visits it, and the node's index either way
    assert P.index_binary_search(vec, 0.0, 6) == (3, 3)
    for i, v in enumerate(vec):
        assert P.fractional_index(v, vec, 6) == i + 1
    assert P.index_binary_search(vec, 0.2, 6) == (3, 4) and P.fractional_index(0.2, vec, 6) == 1 / 0.4 * 0.2 + 3
    # below the first and above the last node: the end pair, extrapolated
    assert P.index_binary_search(vec, -1.7, 6) == (1, 2) and P.index_binary_search(vec, 1.6, 6) == (5, 6)
    assert P.fractional_index(-1.25, vec, 6) == 1 / 0.5 * (-0.25) + 1 == 0.5
    assert P.fractional_index(1.6, vec, 6) == 1 / (1 - 0.7) * (1.6 - 0.7) + 5
    # Flat: no index, interpolator (1, 1, 0)
    im, ip, xi = P.interpolator(None, 3)
    assert im.tolist() == ip.tolist() == [1, 1, 1] and not xi.any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. drogued particles
# ---------------------------------------------------------------------------------------------------------------------
def test_drogued_particles_move_with_the_velocity_at_their_depth(ocn):
    """u = z at its nodes (linear: interpolation returns the depth within rounding), v = 0, w = 1: a drogued particle keeps z although
    w = 1 and advances by depth * Δt in x; the free one advances by its own z"""
    grid = _grid(ocn, False)
    g = P.Geometry.of_grid(grid)
    u, _ = _sample(grid, (ocn.Face, ocn.Center, ocn.Center), lambda x, y, z: z + 0 * x)
    v, _ = _sample(grid, (ocn.Center, ocn.Face, ocn.Center), lambda x, y, z: 0 * x)
    w, _ = _sample(grid, (ocn.Center, ocn.Center, ocn.Face), lambda x, y, z: 1 + 0 * x)
    x0, y0, z0, depths = np.array([0.1, -0.4]), np.array([0.2, 0.3]), np.array([0.5, -0.1]), np.array([-0.6, 0.35])
    dt = 0.125
    x, y, z = P.advect(g, x0, y0, z0, u, v, w, dt, 1.0, depths=depths)
    assert np.array_equal(z, z0) and np.array_equal(y, y0)
    assert np.abs(x - (x0 + depths * dt)).max() < 20 * EPS
    xf, _, zf = P.advect(g, x0, y0, z0, u, v, w, dt, 1.0)
    assert np.abs(xf - (x0 + z0 * dt)).max() < 20 * EPS and np.abs(zf - (z0 + dt)).max() < 20 * EPS
    # step: the tracked property uses the particle's own z, not the depth
    Pd = {"x": x0.copy(), "y": y0.copy(), "z": z0.copy(), "s": np.zeros(2)}
    P.step(g, Pd, [("s", u, P.LOC_U)], (u, v, w), dt, 1.0, depths)
    assert np.abs(Pd["s"] - z0).max() < 20 * EPS and np.array_equal(Pd["z"], z0)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the descriptor
# ---------------------------------------------------------------------------------------------------------------------
def test_descriptor_show_and_refusals(ocn):
    n = 10
    p = ocn.LagrangianParticles(x=np.zeros(n), y=np.zeros(n), z=np.zeros(n), dynamics=ocn.DroguedParticleDynamics(np.linspace(-10, 0, n)))
    lines = repr(p).split("\n")
    assert lines[:4] == ["10 LagrangianParticles with eltype Particle:", "├── 3 properties: (:x, :y, :z)",
                         "├── particle-wall restitution coefficient: 1.0", "├── 0 tracked fields: ()"]          # drogued_dynamics.jl:26-29
    assert lines[4].startswith("└── dynamics: DroguedParticleDynamics{")
    q = ocn.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3))
    assert repr(q).split("\n")[4] == "└── dynamics: no_dynamics"
    assert len(q) == 3 and q.size == (3,) and q.summary() == "3 LagrangianParticles with eltype Particle and properties (:x, :y, :z)"
    t = ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.ones(2), restitution=0.5, T=np.zeros(2), tracked_fields={"T": "T"})
    assert "├── 1 tracked fields: (:T,)" in repr(t) and "4 properties: (:x, :y, :z, :T)" in repr(t) and "coefficient: 0.5" in repr(t)
    assert np.array_equal(t.z, np.ones(2)) and np.array_equal(t.set(z=[2.0, 3.0]).z, [2.0, 3.0])
    with pytest.raises(ValueError, match="x, y, z must all have the same size!"):
        ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(3), z=np.zeros(2))
    with pytest.raises(ValueError, match=r"x, y, z must have dimension 1 but ndims=\(2, 2, 2\)"):
        ocn.LagrangianParticles(x=np.zeros((2, 2)), y=np.zeros((2, 2)), z=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="T is a tracked field but Particle has no T field!"):
        ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2), tracked_fields={"T": "T"})
    with pytest.raises(NotImplementedError, match="C ABI"):
        ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2), dynamics=lambda particles, model, dt: None)
    with pytest.raises(NotImplementedError, match="computed"):
        ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2), s=np.zeros(2), tracked_fields={"s": lambda u, v: (u * u + v * v) ** 0.5})
    with pytest.raises(ValueError, match="depths"):
        ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2), dynamics=ocn.DroguedParticleDynamics(np.zeros(3)))


def test_model_refusals_need_no_device(ocn):
    """validated before any handle exists: a partitioned grid, a tracked field the model does not have"""
    from test_cabi_and_host import _FakeCtx
    from oldoceananigans_jl_amd import distributed as dist
    p = ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2))
    part = dist.DistributedRectilinearGrid(_FakeCtx(2, 0), size=(16, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=part, particles=p)
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    s = ocn.LagrangianParticles(x=np.zeros(2), y=np.zeros(2), z=np.zeros(2), s=np.zeros(2), tracked_fields={"s": "salt"})
    with pytest.raises(ValueError, match="no field salt"):
        ocn.NonhydrostaticModel(grid=grid, particles=s)
    with pytest.raises(TypeError):
        ocn.NonhydrostaticModel(grid=grid, particles=(np.zeros(2),) * 3)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the bounds requirement, on the host build of the kernel's index function
# ---------------------------------------------------------------------------------------------------------------------
def _host_indices(N, H, topo, face, first, spacing, nodes, coordinate):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    coordinate = np.ascontiguousarray(coordinate, dtype=np.float64)
    n = coordinate.size
    idx, w = np.zeros(2 * n, dtype=np.int32), np.zeros(n)
    tab = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.float64)
    rc = L.ocn_particle_indices_host(N, H, topo, int(face), float(first), float(spacing), None if tab is None else tab.ctypes.data_as(dp), n,
                                     coordinate.ctypes.data_as(dp), idx.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(dp))
    assert rc == 0
    return idx[0::2].astype(np.int64), idx[1::2].astype(np.int64), w


DIRECTIONS = {
    # name: N, H, topology, face, regular (first node, Δ) or the node table
    "periodic_center": (8, 3, P.PERIODIC, False, (0.0625, 0.125), None),
    "periodic_face": (8, 3, P.PERIODIC, True, (0.0, 0.125), None),
    "bounded_center": (12, 3, P.BOUNDED, False, (-0.95, 0.1), None),
    "bounded_face": (12, 3, P.BOUNDED, True, (-1.0, 0.1), None),
    "stretched_center": (5, 3, P.BOUNDED, False, None, [-0.75, -0.25, 0.2, 0.55, 0.85]),
    "stretched_face": (5, 3, P.BOUNDED, True, None, STRETCHED),
    "flat": (1, 0, P.FLAT, False, (0.0, 1.0), None),
}


@pytest.mark.parametrize("name", list(DIRECTIONS))
def test_corner_indices_stay_inside_the_parent_array(name):
    """NaN, ±Inf, ±1e300 and one cell outside the halo: every corner index lies in [1 - H, N + H (+ 1 for a Face that ends in a wall)];
    1000 random positions inside the domain: the indices and ξ equal the unclamped restatement"""
    N, H, topo, face, regular, nodes = DIRECTIONS[name]
    first, spacing = regular if regular else (nodes[0], 1.0)
    lo, hi = 1 - H, N + H + (1 if (face and topo == P.BOUNDED) else 0)
    x0 = first if regular else nodes[0]
    d = spacing if regular else (nodes[1] - nodes[0])
    xN = x0 + N * spacing if regular else nodes[-1]
    wild = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, x0 - (H + 1.5) * d, xN + (H + 2.5) * d, 2.0 ** 40, -2.0 ** 40])
    im, ip, w = _host_indices(N, H, topo, face, first, spacing, nodes, wild)
    assert im.min() >= lo and im.max() <= hi and ip.min() >= lo and ip.max() <= hi, (im, ip)
    assert np.all((ip == im + 1) | (ip == hi))
    if topo == P.FLAT:
        assert im.tolist() == ip.tolist() == [1] * len(wild) and not w.any()
        return
    g = P.Geometry((1, 1, N), (0, 0, H), (P.FLAT, P.FLAT, topo), (0, 0, first), (0, 0, first), (1, 1, spacing), (0, 0, 0), (0, 0, 0),
                   zf=nodes if (nodes and face) else None, zc=nodes if (nodes and not face) else None)
    x = np.random.default_rng(8).uniform(x0, xN, 1000)
    im, ip, w = _host_indices(N, H, topo, face, first, spacing, nodes, x)
    rm, rp, rw = P.interpolator(P.fractional_indices(g, 2, face, x))
    assert np.array_equal(im, rm) and np.array_equal(ip, rp) and np.array_equal(w, rw)
    # within one halo cell of the domain the clamp changes nothing either
    edge = np.array([x0 - 0.9 * d, xN + 0.4 * d]) if regular else np.array([nodes[0] - 0.4 * d, nodes[-1] + 0.1])
    im, ip, w = _host_indices(N, H, topo, face, first, spacing, nodes, edge)
    rm, rp, rw = P.interpolator(P.fractional_indices(g, 2, face, edge))
    assert np.array_equal(im, rm) and np.array_equal(ip, rp) and np.array_equal(w, rw)
