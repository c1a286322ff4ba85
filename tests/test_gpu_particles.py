"""particles = LagrangianParticles on the MI355X against the numpy restatement (tests/particles_reference.py, pinned on the CPU by
tests/test_particles_host.py):
  * the raw kernels == the restatement (np.array_equal): interpolate at four locations, advect_particles with wraps, bounces and clamps for
    three restitutions, with and without depths, on four grids, 257 particles (one over a block);
  * the model (RK3 and AB2, three steps) against ParticlesOrchestrated: fields 1e-12, positions 1e-12 of the domain length, tracked
    properties 1e-12 of the field's scale;
  * fuse_substep, use_graph and fused_epilogue leave the particles' bits alone;
  * set / replace / set a property / clear on a live model; zero particles;
  * the reference's uniform-flow test (test_lagrangian_particle_tracking.jl:107-196), with the background v;
  * a checkpoint with particles; the refusals of the C entry points."""
import ctypes as C

import numpy as np
import pytest

from helpers import rel_err, smooth_state, tanh_faces
import particles_reference as P

pytestmark = pytest.mark.gpu

CASES = {
    "ppb_stretched": dict(size=(8, 6, 10), topo=("Periodic", "Periodic", "Bounded"), stretched=True),
    "pfb": dict(size=(8, 8), topo=("Periodic", "Flat", "Bounded"), stretched=False),
    "bbb": dict(size=(12, 10, 8), topo=("Bounded", "Bounded", "Bounded"), stretched=False),
    "ppp": dict(size=(8, 8, 8), topo=("Periodic", "Periodic", "Periodic"), stretched=False),
}
N_PARTICLES = 257           # one over a block of 256: the tail block is live


def _grids(ocn, oracle, arch, name):
    c = CASES[name]
    topo = c["topo"]
    Nz = c["size"][-1]
    z = tanh_faces(Nz) if c["stretched"] else (-1.0, 0.0)
    kw = {d: (0.0, 1.0) for d, t in zip("xy", topo) if t != "Flat"}
    grid = ocn.RectilinearGrid(arch, size=c["size"], topology=tuple(getattr(ocn, t) for t in topo), z=z, **kw)
    g_cpu = None
    if oracle is not None:
        g_cpu = oracle.Grid(tuple(grid.size), topology=tuple({"Periodic": 0, "Bounded": 1, "Flat": 3}[t] for t in topo), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    return grid, g_cpu


def _positions(grid, g, seed, margin=0.0):
    """257 positions: hand-placed ones -- on nodes, on xᴸ and xᴿ, inside the first and the last half cell (where the halo is read) -- and
    random interior ones; margin > 0 keeps every one that far from the faces"""
    rng = np.random.default_rng(seed)
    out = []
    for d in range(3):
        lo, hi, L = g.xL[d], g.xR[d], g.length(d)
        if g.topo[d] == P.FLAT:
            out.append(np.full(N_PARTICLES, lo))
            continue
        dl = g.d[d] if not (d == 2 and g.zf is not None) else g.zf[1] - g.zf[0]
        dh = g.d[d] if not (d == 2 and g.zf is not None) else g.zf[-1] - g.zf[-2]
        special = [lo + 0.2 * dl, lo + 0.45 * dl, hi - 0.3 * dh, hi - 0.05 * dh, lo + 1.5 * dl, lo + 2.0 * dl, lo + dl, hi - dh]
        if margin == 0.0:
            special += [lo, hi]
        special = np.array(special)
        a = rng.uniform(lo + max(margin, 0.0), hi - max(margin, 0.0), N_PARTICLES)
        where = rng.permutation(N_PARTICLES)[:len(special)]          # per direction at other particles: every mix with interior values occurs
        a[where] = special
        if margin > 0.0:
            a = np.clip(a, lo + margin, hi - margin)
        out.append(a)
    return out


def _fields(ocn, grid, seed, names):
    """O(1) smooth values plus noise over the WHOLE parent array -> (dict name -> Field, dict name -> parent array)"""
    rng = np.random.default_rng(seed)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}
    flds, parents = {}, {}
    for q, n in enumerate(names):
        f = make[n](grid)
        I, J, K = np.ogrid[:f.shape[0], :f.shape[1], :f.shape[2]]
        a = 0.6 * np.sin(0.7 * I + seed + q) * np.cos(0.5 * J + 0.2 * q) + 0.4 * np.cos(0.9 * K + 0.3 * I) + 0.05 * rng.standard_normal(f.shape)
        a = np.asfortranarray(a)
        f.set_parent(a)
        flds[n], parents[n] = f, a
    return flds, parents


# ---------------------------------------------------------------------------------------------------------------------
# 1. the raw kernels == the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_interpolate_is_the_restatement(ocn, arch, name):
    grid, _ = _grids(ocn, None, arch, name)
    g = P.Geometry.of_grid(grid)
    x, y, z = _positions(grid, g, 11)
    F, A = _fields(ocn, grid, 3, "uvwc")
    for n, loc in (("c", P.LOC_C), ("u", P.LOC_U), ("v", P.LOC_V), ("w", P.LOC_W)):
        got = ocn.kernels.interpolate(grid, F[n], x, y, z)
        want = P.interpolate(g, A[n], loc, x, y, z)
        assert np.all(np.isfinite(got)) and np.array_equal(got, want), (name, n, np.abs(got - want).max())


@pytest.mark.parametrize("drogued", [False, True])
@pytest.mark.parametrize("Cr", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("name", list(CASES))
def test_advect_particles_is_the_restatement(ocn, arch, name, Cr, drogued):
    """velocities of O(1) and Δt = 2.5: displacements up to two and a half domain lengths, so particles wrap (also more than once), bounce
    and hit the clamp at the far wall"""
    grid, _ = _grids(ocn, None, arch, name)
    g = P.Geometry.of_grid(grid)
    x, y, z = _positions(grid, g, 12)
    depths = _positions(grid, g, 13)[2] if drogued else None
    F, A = _fields(ocn, grid, 5, "uvw")
    dt = 2.5
    got = ocn.kernels.advect_particles(grid, x, y, z, F["u"], F["v"], F["w"], dt, restitution=Cr, depths=depths)
    want = P.advect(g, x, y, z, A["u"], A["v"], A["w"], dt, Cr, depths)
    moved = {}
    for n, a, b, start in zip("xyz", got, want, (x, y, z)):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), (name, Cr, drogued, n, np.abs(a - b).max())
        moved[n] = a != start
    assert np.array_equal(got[2], z) if drogued else (moved["z"].any() or g.topo[2] == P.FLAT)
    # the rules were exercised: positions left the domain before the boundary rule, on both sides
    za = z if depths is None else depths
    raw = x + (P.interpolate(g, A["u"], P.LOC_U, x, y, za) * dt)
    assert (raw > g.xR[0]).any() and (raw < g.xL[0]).any()
    if g.topo[0] == P.BOUNDED and Cr == 1.0:
        assert (got[0] == g.xL[0]).any() or (got[0] == g.xR[0]).any()          # the clamp
    if g.topo[0] == P.PERIODIC:
        assert (raw > g.xR[0] + g.length(0)).any() or (raw < g.xL[0] - g.length(0)).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model against ParticlesOrchestrated
# ---------------------------------------------------------------------------------------------------------------------
NU, KAPPA, FCOR = 2e-3, 5e-3, 0.7
MODEL_CASES = {
    # case: grid, physics (FPlane + BuoyancyTracer + ScalarDiffusivity), background u, drogue, tracked u / w / b
    "plain": ("ppb_stretched", False, False, False, False),
    "background": ("ppb_stretched", False, True, False, False),
    "physics": ("ppb_stretched", True, False, False, False),
    "drogue": ("ppb_stretched", False, False, True, False),
    "tracked": ("ppb_stretched", True, False, False, True),
    "plain_ppp": ("ppp", False, False, False, False),
    "tracked_bbb": ("bbb", False, False, False, True),
    "physics_bbb": ("bbb", True, False, False, True),
    "tracked_ppp": ("ppp", False, False, False, True),
}
STEPS = 3
MARGIN = 0.03               # far more than the particles travel in three steps (|U| Δt STEPS < 0.01), so none comes near a face


def _model_pair(ocn, oracle, arch, case, timestepper, options=None, yardstick=True, particles=True):
    name, physics, background, drogued, tracked = MODEL_CASES[case]
    grid, g_cpu = _grids(ocn, oracle if yardstick else None, arch, name)
    g = P.Geometry.of_grid(grid)
    x, y, z = _positions(grid, g, 21, margin=MARGIN)
    depths = _positions(grid, g, 22, margin=MARGIN)[2] if drogued else None
    props = {"pu": np.zeros(N_PARTICLES), "pw": np.zeros(N_PARTICLES), "pb": np.zeros(N_PARTICLES)} if tracked else {}
    lp = ocn.LagrangianParticles(x=x, y=y, z=z, restitution=0.5, dynamics=ocn.DroguedParticleDynamics(depths) if drogued else None,
                                 tracked_fields={"pu": "u", "pw": "w", "pb": "b"} if tracked else None, **props) if particles else None
    bg = {"u": lambda x, y, z: 0.4 + 0.3 * z + 0 * x + 0 * y} if background else None
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer() if physics else None,
                                    coriolis=ocn.FPlane(f=FCOR) if physics else None,
                                    closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA) if physics else None, background_fields=bg, particles=lp)
    for k, v in (options or {}).items():
        model.set_option(k, v)
    nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
    vals = smooth_state({("T" if n == "b" else n): v for n, v in nodes.items()}, 17)
    vals["b"] = vals.pop("T")
    ocn.set_model(model, **vals)
    yard = None
    if yardstick:
        yard = P.ParticlesOrchestrated(oracle, g_cpu, 1, NU if physics else 0.0, (KAPPA if physics else 0.0,), geometry=g,
                                       particles=dict(x=x, y=y, z=z, **props), restitution=0.5, depths=depths,
                                       tracked={"pu": "u", "pw": "w", "pb": "c0"} if tracked else None,
                                       background={"u": model.background_fields.velocities.u.parent()} if background else None,
                                       buoyancy_index=0 if physics else None, fcor=FCOR if physics else None, closure="numpy")
        yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["b"])
    return grid, g, model, yard


def _step(ocn, model, yard, timestepper, steps, dt):
    for _ in range(steps):
        ocn.time_step(model, dt)
        if yard is not None:
            yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("case", [c for c in MODEL_CASES if c not in ("physics_bbb", "tracked_ppp")])          # (those serve the comparisons below)
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, case, timestepper):
    """three steps. The yardstick first shows, on the CPU, that no particle came within 1e-6 of a domain face at any stage (a wrap or a
    bounce is discontinuous); then fields 1e-12, positions 1e-12 of the domain length, tracked properties 1e-12 of the field's scale"""
    grid, g, model, yard = _model_pair(ocn, oracle, arch, case, timestepper)
    assert model.get_option("particles") == N_PARTICLES
    dt = 0.05 / grid.Nx
    _step(ocn, model, yard, timestepper, STEPS, dt)
    assert yard.min_face_distance > 1e-6, yard.min_face_distance
    core = tuple(slice(h, -h) if h else slice(None) for h in grid.halo_size)
    for gn, cn in zip(("u", "v", "w", "b"), yard.names):
        a, b = model.fields()[gn].parent()[core], yard.U[cn][core]
        assert np.all(np.isfinite(a)) and rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    for d, n in enumerate("xyz"):
        a, b = getattr(model.particles, n), yard.P[n]
        L = g.length(d) if g.topo[d] != P.FLAT else 1.0
        print(f"case {case} {timestepper} {n}: max difference {np.abs(a - b).max():.3e} of length {L}")
        assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 1e-12 * L, (n, np.abs(a - b).max())
    moved = np.abs(model.particles.x - _positions(grid, g, 21, margin=MARGIN)[0]).max()
    assert moved > 1e-4                                   # the particles did move, by far more than the tolerance
    if MODEL_CASES[case][3]:
        assert np.array_equal(model.particles.z, yard.P["z"]) and np.array_equal(yard.P["z"], _positions(grid, g, 21, margin=MARGIN)[2])
    for prop, cn in (("pu", "u"), ("pw", "w"), ("pb", "c0")) if MODEL_CASES[case][4] else ():
        a, b = getattr(model.particles, prop), yard.P[prop]
        scale = np.abs(yard.U[cn]).max()
        print(f"case {case} {timestepper} {prop}: max difference {np.abs(a - b).max():.3e} on the scale {scale:.3e}")
        assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-12 * scale, (prop, np.abs(a - b).max())
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == STEPS
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. options that must give the same bits
# ---------------------------------------------------------------------------------------------------------------------
def _particle_bits(model):
    return {n: getattr(model.particles, n) for n in model.particles.property_names}


def _same_particles(a, b, what):
    pa, pb = _particle_bits(a), _particle_bits(b)
    for n in pa:
        assert np.all(np.isfinite(pa[n])) and np.array_equal(pa[n], pb[n]), (what, n, np.abs(pa[n] - pb[n]).max())


@pytest.mark.parametrize("case", ["tracked", "plain_ppp", "physics_bbb"])
def test_fused_substep_leaves_the_particles_alone(ocn, arch, case):
    """fuse_substep 1: the next substep rides in the tendency launch and U / U2 swap right after update_state! -- the particles must have
    seen the stage's own fields, as with fuse_substep 0"""
    grid, g, fused, _ = _model_pair(ocn, None, arch, case, "RungeKutta3", yardstick=False)
    _, _, plain, _ = _model_pair(ocn, None, arch, case, "RungeKutta3", options={"fuse_substep": 0}, yardstick=False)
    assert fused.get_option("fuse_substep_active") == 1 and plain.get_option("fuse_substep_active") == 0
    for model in (fused, plain):
        _step(ocn, model, None, "RungeKutta3", 3, 0.05 / grid.Nx)
    _same_particles(fused, plain, case)
    for n in fused.fields():
        assert np.array_equal(fused.fields()[n].parent(), plain.fields()[n].parent()), n
    fused.close()
    plain.close()


@pytest.mark.parametrize("case", ["tracked", "plain_ppp"])
def test_captured_graph_leaves_the_particles_alone(ocn, arch, case):
    grid, g, graph, _ = _model_pair(ocn, None, arch, case, "RungeKutta3", options={"use_graph": 1}, yardstick=False)
    _, _, plain, _ = _model_pair(ocn, None, arch, case, "RungeKutta3", options={"use_graph": 0}, yardstick=False)
    for model in (graph, plain):
        _step(ocn, model, None, "RungeKutta3", 5, 0.05 / grid.Nx)
    _same_particles(graph, plain, case)
    graph.close()
    plain.close()


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_fused_epilogue_leaves_the_particles_alone(ocn, arch, timestepper):
    grid, g, default, _ = _model_pair(ocn, None, arch, "tracked", timestepper, yardstick=False)
    _, _, other, _ = _model_pair(ocn, None, arch, "tracked", timestepper, options={"fused_epilogue": 0}, yardstick=False)
    for model in (default, other):
        _step(ocn, model, None, timestepper, 3, 0.05 / grid.Nx)
    _same_particles(default, other, timestepper)
    default.close()
    other.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. life cycle on one live model
# ---------------------------------------------------------------------------------------------------------------------
def _same_fields(a_model, b_model, what):
    for n in a_model.fields():
        for label, get in (("field", lambda m: m.fields()[n]), ("Gn", lambda m: m.tendency(n))):
            a, b = get(a_model).parent(), get(b_model).parent()
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (what, label, n)
    assert np.array_equal(a_model.pressures.pNHS.parent(), b_model.pressures.pNHS.parent()), what


def test_life_cycle_on_a_live_model(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    grid, g, model, _ = _model_pair(ocn, None, arch, "tracked", "RungeKutta3", yardstick=False)
    _, _, never, _ = _model_pair(ocn, None, arch, "tracked", "RungeKutta3", yardstick=False, particles=False)
    assert model.get_option("particles") == N_PARTICLES and never.get_option("particles") == 0 and never.particles is None
    dt = 0.05 / grid.Nx
    for m in (model, never):
        _step(ocn, m, None, "RungeKutta3", 2, dt)
    _same_fields(model, never, "particles do not act on the fields")
    # replace with a different n (the tracked properties go with the old particles)
    a = np.linspace(0.2, 0.8, 5)
    assert L.ocn_model_set_particles(model.handle, 5, a.ctypes.data_as(dp), a.ctypes.data_as(dp), (a - 1).ctypes.data_as(dp), 1.0, None) == 0
    count = C.c_int()
    assert L.ocn_model_particle_count(model.handle, C.byref(count)) == 0 and count.value == 5 and model.get_option("particles") == 5
    out = np.zeros(5)
    assert L.ocn_model_particle_property(model.handle, b"z", out.ctypes.data_as(dp)) == 0 and np.array_equal(out, a - 1)
    assert L.ocn_model_particle_property(model.handle, b"pu", out.ctypes.data_as(dp)) != 0
    # set a property, step, read it back moved
    b = np.full(5, 0.5)
    assert L.ocn_model_set_particle_property(model.handle, b"y", b.ctypes.data_as(dp)) == 0
    for m in (model, never):
        _step(ocn, m, None, "RungeKutta3", 1, dt)
    assert L.ocn_model_particle_property(model.handle, b"y", out.ctypes.data_as(dp)) == 0 and np.all(out != 0.5) and np.all(np.abs(out - 0.5) < 0.01)
    # zero particles: steps, launches nothing for them
    assert L.ocn_model_set_particles(model.handle, 0, a.ctypes.data_as(dp), a.ctypes.data_as(dp), a.ctypes.data_as(dp), 1.0, None) == 0
    assert model.get_option("particles") == 0
    for m in (model, never):
        _step(ocn, m, None, "RungeKutta3", 1, dt)
    # clear: particles = nothing
    assert L.ocn_model_set_particles(model.handle, 0, None, None, None, 1.0, None) == 0
    assert model.get_option("particles") == 0 and L.ocn_model_particle_property(model.handle, b"x", out.ctypes.data_as(dp)) != 0
    for m in (model, never):
        _step(ocn, m, None, "RungeKutta3", 2, dt)
    _same_fields(model, never, "after clearing")
    model.close()
    never.close()


def test_zero_particles_through_the_constructor(ocn, arch):
    grid, _ = _grids(ocn, None, arch, "ppp")
    lp = ocn.LagrangianParticles(x=np.zeros(0), y=np.zeros(0), z=np.zeros(0))
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("b",), particles=lp)
    ocn.set_model(model, u=0.3)
    ocn.time_step(model, 0.01)
    assert len(model.particles) == 0 and model.particles.x.shape == (0,) and model.get_option("particles") == 0
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the reference's uniform-flow test
# ---------------------------------------------------------------------------------------------------------------------
def _approx(a, b):
    return np.all(np.abs(a - b) <= np.sqrt(2.220446049250313e-16) * np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_reference_uniform_flow(ocn, arch, timestepper, background):
    """test_lagrangian_particle_tracking.jl:107-196 on its 5 x 5 x 5 (Periodic, Periodic, Bounded) grid on (-1, 1)³: u = v = 1 (v from the
    background when there is one), Δt = 1e-2, one step: x, y ≈ 0.01, z ≈ 0.5, tracked u ≈ 1, v ≈ 1 (the model's own: 0 with a background),
    w ≈ 0"""
    grid = ocn.RectilinearGrid(arch, size=(5, 5, 5), x=(-1, 1), y=(-1, 1), z=(-1, 1), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    n = 10
    lp = ocn.LagrangianParticles(x=np.zeros(n), y=np.zeros(n), z=np.full(n, 0.5), u=np.zeros(n), v=np.zeros(n), w=np.zeros(n),
                                 tracked_fields={"u": "u", "v": "v", "w": "w"})
    model = ocn.NonhydrostaticModel(grid=grid, tracers=(), timestepper=timestepper, particles=lp,
                                    background_fields={"v": lambda x, y, z: 1.0 + 0 * x + 0 * y + 0 * z} if background else None)
    ocn.set_model(model, u=1.0) if background else ocn.set_model(model, u=1.0, v=1.0)
    ocn.time_step(model, 1e-2)
    p = model.particles
    assert len(p) == n and p.size == (n,) and p.property_names == ("x", "y", "z", "u", "v", "w")
    assert _approx(p.x, 0.01) and _approx(p.y, 0.01) and _approx(p.z, 0.5)
    assert _approx(p.u, 1.0) and np.all(np.abs(p.w) < 1e-12)
    assert np.all(np.abs(p.v) < 1e-12) if background else _approx(p.v, 1.0)
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. checkpoint with particles
# ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_with_particles(ocn, arch, tmp_path):
    """on the triply periodic grid, where a restored model continues bit for bit (on a Bounded z the tridiagonal solver keeps its previous
    solution in the singular column and a restart agrees to round-off, checkpointer.py)"""
    from oldoceananigans_jl_amd.checkpointer import ADDRESS, set_from_checkpoint, write_checkpoint
    grid, g, model, _ = _model_pair(ocn, None, arch, "tracked_ppp", "RungeKutta3", yardstick=False)
    dt = 0.05 / grid.Nx
    _step(ocn, model, None, "RungeKutta3", 2, dt)
    path = write_checkpoint(model, str(tmp_path / "with_particles"))
    with np.load(path) as file:
        assert sorted(k for k in file if "/particles/" in k) == sorted(f"{ADDRESS}/particles/{n}" for n in ("x", "y", "z", "pu", "pw", "pb"))
    _, _, fresh, _ = _model_pair(ocn, None, arch, "tracked_ppp", "RungeKutta3", yardstick=False)
    set_from_checkpoint(fresh, path)
    _same_particles(fresh, model, "restored")
    for m in (model, fresh):
        _step(ocn, m, None, "RungeKutta3", 2, dt)
    _same_particles(fresh, model, "after two more steps")
    _same_fields(fresh, model, "after two more steps")
    # a model without particles writes exactly the entries it wrote before
    _, _, without, _ = _model_pair(ocn, None, arch, "tracked_ppp", "RungeKutta3", yardstick=False, particles=False)
    with np.load(write_checkpoint(without, str(tmp_path / "without"))) as file:
        assert not [k for k in file if "particles" in k]
    for m in (model, fresh, without):
        m.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ocn, arch):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    EINVAL = -1
    grid, g, model, _ = _model_pair(ocn, None, arch, "tracked", "RungeKutta3", yardstick=False)
    a = np.full(4, 0.5)
    A = a.ctypes.data_as(dp)
    assert L.ocn_model_set_particles(None, 4, A, A, A, 1.0, None) == EINVAL
    assert L.ocn_model_set_particles(model.handle, -1, A, A, A, 1.0, None) == EINVAL
    assert L.ocn_model_set_particles(model.handle, 4, A, None, A, 1.0, None) == EINVAL
    assert L.ocn_model_set_particles(model.handle, 4, None, None, None, 1.0, None) == EINVAL
    assert L.ocn_model_track_particle_field(model.handle, b"q", b"salt") == EINVAL
    assert L.ocn_model_track_particle_field(model.handle, b"q", b"Gu") == EINVAL
    assert L.ocn_model_track_particle_field(model.handle, b"x", b"u") == EINVAL
    assert L.ocn_model_track_particle_field(model.handle, None, b"u") == EINVAL
    for q in range(5):                                    # pu, pw, pb are tracked: five more make eight
        assert L.ocn_model_track_particle_field(model.handle, b"extra%d" % q, b"v") == 0
    assert L.ocn_model_track_particle_field(model.handle, b"ninth", b"v") == EINVAL
    assert b"at most 8" in L.ocn_last_error()
    assert L.ocn_model_track_particle_field(model.handle, b"extra0", b"w") == 0          # naming a property again replaces its field
    assert model.get_option("particles") == N_PARTICLES               # every refused call left the particles where they were
    assert np.array_equal(model.particles.x, _positions(grid, g, 21, margin=MARGIN)[0])
    out = C.c_void_p()
    assert L.ocn_malloc(C.byref(out), 8 * 3) == 0
    assert L.ocn_interpolate_at(grid.handle, -1, out, out, out, model.velocities.u.data, _lib.i3((1, 0, 0)), out) == EINVAL
    assert L.ocn_interpolate_at(grid.handle, 3, out, out, None, model.velocities.u.data, _lib.i3((1, 0, 0)), out) == EINVAL
    assert L.ocn_advect_particles(grid.handle, 3, out, out, out, None, 1.0, 0.1, model.velocities.u.data, None, model.velocities.w.data) == EINVAL
    L.ocn_free(out)
    model.close()


def test_partitioned_handles_refuse_particles(ocn, arch):
    """OCN_ENOTSUP (-2) on a partitioned handle (one rank that is its own neighbour); `particles` keeps answering 0"""
    from oldoceananigans_jl_amd import _lib
    from oldoceananigans_jl_amd import distributed as dist
    L = _lib.lib()
    uid = C.create_string_buffer(128)
    _lib.check(L.ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    grid = dist.DistributedRectilinearGrid(ctx, size=(8, 8, 8), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    part = dist.LibraryDistributedModel(grid=grid, tracers=())
    a = np.full(4, 0.5)
    A = a.ctypes.data_as(C.POINTER(C.c_double))
    assert L.ocn_model_set_particles(part.handle, 4, A, A, A, 1.0, None) == -2 and b"partitioned" in L.ocn_last_error()
    assert part.get_option("particles") == 0
    with pytest.raises(NotImplementedError, match="partitioned"):
        dist.LibraryDistributedModel(grid=grid, tracers=(), particles=ocn.LagrangianParticles(x=a, y=a, z=a - 1))
    part.close()
    ctx.close()
