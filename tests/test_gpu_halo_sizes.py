"""GPU: the kernel paths at halo sizes other than (3, 3, 3). Every test is parametrized over halo_cases.HALOS -- three asymmetric halos,
in which every direction takes each of three distinct values, so Hx, Hy, Hz used in each other's place, a parent stride built from the
wrong halo or a literal 3 where a halo was meant changes the result; and (7, 7, 7), where H <= N < 2H on the small grids.

The reference is the oracle AT THE SAME HALO: tests/test_halo_sizes_host.py shows on the CPU that the oracle's interiors do not depend on
the halo depth. No tolerance is new: `==` where the suite asserts `==` at (3, 3, 3) (halo fills, tendencies, option variants against the
default options), helpers.rel_err < 1e-12 after steps, pNHS with the error model of test_gpu_option_variants.py. Interiors are taken with
halo_cases.interior from the grid's own halo.

  1. halo fills: whole parent arrays against the oracle's fill, default and Value / Gradient / Open / Flux conditions (constant and
     array-valued), both fused_halo values;
  2. tendencies: every tendency_impl, 0 / 2 / 3 tracers, chunk lengths with a first chunk above plane 0 and a chunk seam, z-windows off,
     the contracted arithmetic; the interiors also equal the device's own at (3, 3, 3);
  3. pressure solvers on their own, and solve_for_pressure with every solver variant and its *_active read-back;
  4. time steps: RK3 and AB2 against the oracle, option variants and graph replay bit-identical, the folded pressure step against the
     separate kernels on whole parent arrays, checkpoint / restore; the difference of the stepped fields from the (3, 3, 3) run is printed;
  6. one smallest case per feature kernel (diagnostics, forcing and boundary functions, table forcings, particles, the vertically implicit
     solve and model, Smagorinsky, Stokes drift, background fields, PerturbationAdvection open boundaries, tilted gravity) against its numpy
     restatement at that halo;
  7. the partitioned model inside the library on virtual ranks and on the RCCL self-loop, at (5, 3, 4) and (4, 6, 3): slabs, irregular slabs,
     a Bounded partitioned x, pencils, thin_halos / async_halos / early_exchange / strip_width variants, against the serial oracle.

Every stepping case prints its worst relative error."""
import contextlib

import numpy as np
import pytest

import halo_cases as HC
from helpers import rel_err, smooth_state
from test_gpu_reference_tests import approx, laplacian

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
CNAMES = ["u", "v", "w", "c0", "c1", "c2"]
TRACERS = ("T", "S", "C3")
LIBRARY_DEFAULTS = {"fused_halo": 1, "real_fft": 1, "c2r_strided": 1, "fused_zfft": 1, "tendency_impl": 2, "arithmetic": 0, "role_kchunk": 0,
                    "fused_kchunk": 0, "fused_zwin": 1}
halos = pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_models():
    yield
    for v in _cache.values():
        for m in (v if isinstance(v, tuple) else (v,)):
            if hasattr(m, "close") and hasattr(m, "fields"):
                m.close()
    _cache.clear()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@contextlib.contextmanager
def _options(target, opts):
    """set the options on a model or as library defaults (the package); afterwards back to the library's defaults"""
    try:
        for k, v in opts.items():
            target.set_option(k, v)
        yield
    finally:
        for k in opts:
            target.set_option(k, LIBRARY_DEFAULTS[k])


def _tag(opts):
    return "-".join("%s=%d" % kv for kv in opts.items()) or "default"


def _ids(v):
    if isinstance(v, dict):
        return _tag(v)
    if isinstance(v, tuple):
        return "".join(s[0] for s in v) if isinstance(v[0], str) else "x".join(map(str, v))
    return str(v)


def _grids(ocn, oracle, arch, gid, halo):
    topology, size, stretched = HC.GRIDS[gid]
    return _cached(("grids", gid, halo), lambda: (HC.make_grid(ocn, arch, topology, size, halo, stretched),
                                                  HC.make_oracle_grid(oracle, topology, size, halo, stretched)))


def _locs(ocn):
    F, Cn = ocn.Face, ocn.Center
    return {"u": (F, Cn, Cn), "v": (Cn, F, Cn), "w": (Cn, Cn, F), "T": (Cn,) * 3, "S": (Cn,) * 3, "C3": (Cn,) * 3, "pNHS": (Cn,) * 3}


# ---------------------------------------------------------------------------------------------------------------------
# 1. halo fills
# ---------------------------------------------------------------------------------------------------------------------
FILL_TOPOLOGIES = HC.ALL_TOPOLOGIES + [HC.PFB]
# the BC_SETS of test_gpu_parity.py
BC_SETS = {
    "c": dict(west=("Value", 1.5), east=("Gradient", -0.7), south=("Gradient", 0.3), north=("Value", -2.0),
              bottom=("Value", 0.25), top=("Flux", 4.0)),
    "u": dict(south=("Value", 0.0), north=("Gradient", 0.1), bottom=("Value", 0.0), top=("Flux", -1e-3), west=("Open", 0.2)),
    "w": dict(west=("Gradient", 0.5), north=("Value", 1.0), top=("Open", 0.125), bottom=("Open", -0.25)),
}
SIDE_DIR = {"west": 0, "east": 0, "south": 1, "north": 1, "bottom": 2, "top": 2}


def _field_makers(ocn):
    return {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}


def _fill_size(topology, size):
    return tuple(1 if t == "Flat" else n for n, t in zip(size, topology))


@halos
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("size", HC.FILL_SIZES, ids=_ids)
@pytest.mark.parametrize("topology", FILL_TOPOLOGIES, ids=_ids)
def test_halo_fills_with_default_conditions(ocn, oracle, arch, topology, size, fused, halo):
    """random data everywhere, halos included: the whole parent array of u, v, w and a tracer equals the oracle's fill at the same halo"""
    size = _fill_size(topology, size)
    grid = HC.make_grid(ocn, arch, topology, size, halo)
    g_cpu = HC.make_oracle_grid(oracle, topology, size, halo)
    rng = np.random.default_rng(7)
    with _options(ocn, {"fused_halo": fused}):
        for name, make in _field_makers(ocn).items():
            f = make(grid)
            assert f.shape == grid.total_size(f.loc) == g_cpu.parent_size(HC.face_code(ocn, f.loc))
            a = rng.standard_normal(f.shape)
            f.set_parent(a)
            b = np.asfortranarray(a.copy())
            for fill_open in (False, True):
                ocn.fill_halo_regions(f, fill_open_bcs=fill_open)
                g_cpu.fill_halo_regions(b, HC.face_code(ocn, f.loc), fill_open)
                got = f.parent()
                assert np.array_equal(got, b), (name, fill_open, int((got != b).sum()))
            assert not np.array_equal(got, a), name


def _conditions(ocn, rng, topology, grid, key, arrays):
    """the BC_SETS entry of a location on the Bounded sides of the topology; arrays: every value becomes a seeded random array over the
    boundary's interior points (tracers and the Open conditions of w on z, like test_array_valued_boundary_conditions_bit_exact)"""
    spec = {s: kv for s, kv in BC_SETS[key].items() if topology[SIDE_DIR[s]] == "Bounded"}
    if arrays:
        N = grid.size
        tang = {0: (N[1], N[2]), 1: (N[0], N[2]), 2: (N[0], N[1])}
        if key == "w":
            spec = {s: kv for s, kv in spec.items() if SIDE_DIR[s] == 2}
        spec = {s: (k, v + 0.1 * rng.standard_normal(tang[SIDE_DIR[s]])) for s, (k, v) in spec.items()}
    gpu = ocn.FieldBoundaryConditions(**{s: ocn.BoundaryCondition(k, v) for s, (k, v) in spec.items()})
    cpu = {s: (k.lower(), v) for s, (k, v) in spec.items()}
    return spec, gpu, cpu


@halos
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("arrays", [False, True], ids=["constant", "array"])
@pytest.mark.parametrize("size", HC.FILL_SIZES, ids=_ids)
@pytest.mark.parametrize("topology", [HC.BBB, HC.PPB, HC.BPB], ids=_ids)
def test_halo_fills_with_boundary_conditions(ocn, oracle, arch, topology, size, arrays, fused, halo):
    """Value, Gradient, Open and Flux conditions, constant and array-valued (BBB: the per-side kernels; PPB: the one-launch fill): whole parent
    arrays against the oracle's fill, and the flux divergence of the Flux sides on a tendency array"""
    grid = HC.make_grid(ocn, arch, topology, size, halo, stretched=True)
    g_cpu = HC.make_oracle_grid(oracle, topology, size, halo, stretched=True)
    rng = np.random.default_rng(21)
    makers = _field_makers(ocn)
    with _options(ocn, {"fused_halo": fused}):
        for key in (("c", "w") if arrays else ("c", "u", "w")):
            spec, gpu, cpu = _conditions(ocn, rng, topology, grid, key, arrays)
            f = makers[key](grid)
            loc = HC.face_code(ocn, f.loc)
            a = rng.standard_normal(f.shape)
            for fill_open in (False, True):
                f.set_parent(a)
                b = np.asfortranarray(a.copy())
                ocn.fill_halo_regions(f, fill_open_bcs=fill_open, boundary_conditions=gpu)
                g_cpu.fill_halo_regions(b, loc, fill_open, bcs=cpu)
                got = f.parent()
                assert np.array_equal(got, b), (key, fill_open, sorted(spec), int((got != b).sum()))
            if key != "w" and any(k == "Flux" for k, _ in spec.values()):
                G = makers[key](grid)
                ga = rng.standard_normal(G.shape)
                G.set_parent(ga)
                gb = np.asfortranarray(ga.copy())
                ocn.compute_flux_bcs(G, gpu)
                g_cpu.compute_flux_bcs(gb, loc, cpu)
                assert np.array_equal(G.parent(), gb), key
                assert not np.array_equal(gb, ga)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tendencies
# ---------------------------------------------------------------------------------------------------------------------
def _tendency_pair(ocn, oracle, arch, gid, halo, ntr):
    """one model per (grid, halo, tracer count) on a seeded random state, set identically on the oracle, WITHOUT the projection (the FFTs differ
    at round-off; tendencies need identical inputs, as in test_tendencies_match_oracle) -> (model, the oracle's G parent arrays)"""
    def make():
        g_gpu, g_cpu = _grids(ocn, oracle, arch, gid, halo)
        m_gpu = ocn.NonhydrostaticModel(grid=g_gpu, advection=ocn.WENO(), tracers=TRACERS[:ntr])
        assert m_gpu.grid.halo_size == g_gpu.halo_size                      # nothing to inflate: the halo holds the scheme's buffer
        m_cpu = oracle.Model(g_cpu, ntr)
        rng = np.random.default_rng(11 + ntr)
        vals = {n: rng.standard_normal(g_gpu.interior_size(f.loc)) for n, f in m_gpu.fields().items()}        # the same values at every halo
        ocn.set_model(m_gpu, enforce_incompressibility=False, **vals)
        m_cpu.set(enforce_incompressibility=False, **{cn: vals[n] for cn, n in zip(CNAMES, m_gpu.fields())})
        m_cpu.update_state(True)
        ref = {n: m_cpu.field("G" + cn).copy() for cn, n in zip(CNAMES, m_gpu.fields())}
        return m_gpu, ref
    return _cached(("tend", gid, halo, ntr), make)


def _compute_G(ocn, m_gpu, opts):
    with _options(m_gpu, opts):
        active = m_gpu.get_option("fused_tendency_active")
        for n in m_gpu.fields():
            m_gpu.tendency(n).set_parent(np.full(m_gpu.tendency(n).shape, SENTINEL))
        ocn.update_state(m_gpu, True)
        return {n: m_gpu.tendency(n).parent() for n in m_gpu.fields()}, active


def _tendency_cases():
    cases = []
    for gid, (_topology, size, _stretched) in HC.GRIDS.items():
        for ntr in (2, 0, 3):
            cases += [(gid, ntr, {"tendency_impl": impl}) for impl in (0, 1, 2)]
        # the two marching kernels: a first chunk with pb > 0 (Hz > 3), a seam inside the grid (3, 5), one chunk (Nz)
        for kc in (3, 5, size[2]):
            cases += [(gid, 2, {"tendency_impl": 2, "role_kchunk": kc}), (gid, 2, {"tendency_impl": 1, "fused_kchunk": kc})]
        cases += [(gid, 2, {"tendency_impl": 1, "fused_zwin": 0}), (gid, 2, {"tendency_impl": 1, "fused_zwin": 0, "fused_kchunk": 3}),
                  (gid, 2, {"tendency_impl": 1, "fused_zwin": 1, "fused_kchunk": 3})]
    return cases


@halos
@pytest.mark.parametrize("gid,ntr,opts", _tendency_cases(), ids=_ids)
def test_tendencies_are_bit_identical_to_the_oracle(ocn, oracle, arch, gid, ntr, opts, halo):
    """the tendency arrays carry a sentinel: what the kernel wrote equals the oracle at the same halo bit for bit, and the kernel wrote every
    value the oracle computes (elsewhere the oracle's arrays hold their zeros: halos, the wall faces)"""
    m_gpu, ref = _tendency_pair(ocn, oracle, arch, gid, halo, ntr)
    got, active = _compute_G(ocn, m_gpu, opts)
    if gid in ("ppp", "ppb") and opts["tendency_impl"] != 0:
        assert active == 1, (gid, halo, opts)            # the flux-sharing kernels serve these grids at every halo: no fallback
    size = HC.GRIDS[gid][1]
    for n, a in got.items():
        assert a.shape == ref[n].shape
        written = a != SENTINEL
        assert written.sum() >= np.prod(size) - size[0] * size[1], (n, int(written.sum()))
        assert np.array_equal(a[written], ref[n][written]), (gid, halo, ntr, opts, n, int((a[written] != ref[n][written]).sum()))
        assert not ref[n][~written].any(), (gid, halo, ntr, opts, n, "values the oracle computes were not written", int((ref[n][~written] != 0).sum()))


@halos
@pytest.mark.parametrize("gid", ["ppp", "ppb"])
def test_contracted_arithmetic_moves_a_tendency_by_round_off_only(ocn, oracle, arch, gid, halo):
    """arithmetic = 1 with the bound of test_gpu_arithmetic_mode.py::test_one_tendency_evaluation_moves_by_round_off_only: within 2e-14 of
    max|G|, and not identical -- the mode ran"""
    m_gpu, ref = _tendency_pair(ocn, oracle, arch, gid, halo, 2)
    got, active = _compute_G(ocn, m_gpu, {"tendency_impl": 2, "arithmetic": 1})
    assert active == 1
    differs = False
    for n, a in got.items():
        written = a != SENTINEL
        err = np.abs(a[written] - ref[n][written]).max() / np.abs(ref[n]).max()
        print(gid, HC.halo_id(halo), "arithmetic=1", n, "err / max|G|", err)
        assert err < 2e-14, (n, err)
        differs = differs or not np.array_equal(a[written], ref[n][written])
    assert differs


@halos
@pytest.mark.parametrize("gid", list(HC.GRIDS))
def test_tendency_interiors_equal_those_at_halo_3(ocn, oracle, arch, gid, halo):
    """device against device: the interiors of G at halo H equal those of the same library at (3, 3, 3) (both equal the oracle, whose
    interiors do not depend on the halo -- asserted here directly, on the arrays of the default-option launches)"""
    locs = _locs(ocn)
    base_model, base_ref = _tendency_pair(ocn, oracle, arch, gid, HC.BASE, 2)
    model, ref = _tendency_pair(ocn, oracle, arch, gid, halo, 2)
    base = _cached(("G-base", gid), lambda: _compute_G(ocn, base_model, {})[0])
    got = _compute_G(ocn, model, {})[0]
    for n in got:
        a, b = HC.interior(model.grid, got[n], locs[n]), HC.interior(base_model.grid, base[n], locs[n])
        assert a.shape == b.shape and np.abs(b).max() > 0 and not (b == SENTINEL).all()
        assert np.array_equal(a, b), (gid, halo, n, int((a != b).sum()))
        assert np.array_equal(HC.interior(model.grid, ref[n], locs[n]), HC.interior(base_model.grid, base_ref[n], locs[n])), (gid, halo, n)


# ---------------------------------------------------------------------------------------------------------------------
# 3. pressure solvers
# ---------------------------------------------------------------------------------------------------------------------
SOLVER_SIZES = [(16, 16, 16), (11, 16, 7), (8, 13, 27)]


@halos
@pytest.mark.parametrize("size", SOLVER_SIZES, ids=_ids)
@pytest.mark.parametrize("kind,topology", [("fft", t) for t in HC.ALL_TOPOLOGIES] + [("tridiagonal", t) for t in HC.ALL_TOPOLOGIES if t[2] == "Bounded"],
                         ids=_ids)
def test_poisson_solvers_on_their_own(ocn, oracle, arch, kind, topology, size, halo):
    """FFTBasedPoissonSolver on all eight topologies, FourierTridiagonalPoissonSolver on the four with a Bounded stretched z: the solution
    within 1e-12 of the oracle's solver at the same halo (test_poisson_solvers_all_topologies), and its discrete Laplacian -- numpy on the
    filled parent array -- is the source (test_gpu_reference_tests.py)"""
    rng = np.random.default_rng(17)
    stretched = kind == "tridiagonal"
    grid = HC.make_grid(ocn, arch, topology, size, halo, stretched)
    g_cpu = HC.make_oracle_grid(oracle, topology, size, halo, stretched)
    solver = ocn.FFTBasedPoissonSolver(grid) if kind == "fft" else ocn.FourierTridiagonalPoissonSolver(grid)
    s_cpu = oracle.PoissonSolver(g_cpu, 0 if kind == "fft" else 1)
    R = rng.standard_normal(size)
    R -= R.mean()
    dz = 1.0
    if stretched:          # both sides take the Δzᶜ-weighted source (solve_for_pressure.jl:36-42); compatible: Σ = 0
        dz = np.diff(np.asarray(HC.zcoord(topology, size, True)))[None, None, :]
        R = R * dz
        R -= R.mean()
    solver.set_source_term(R)
    s_cpu.rhs[...] = R
    phi = ocn.CenterField(grid)
    phi.set_parent(np.full(phi.shape, SENTINEL))
    ocn.solve(phi, solver)
    p_cpu = g_cpu.zeros((0, 0, 0))
    s_cpu.solve(p_cpu)
    got, want = HC.interior(grid, phi.parent()), HC.interior(g_cpu, p_cpu)
    e = rel_err(got, want)
    print(kind, topology, size, HC.halo_id(halo), "rel err", e)
    assert e < 1e-12, (kind, topology, size, halo, e)
    assert approx(laplacian(ocn, grid, phi), R / dz), (kind, topology, size, halo)
    solver.close()


def _solver_paths(ocn, grid):
    model = ocn.NonhydrostaticModel(grid=grid, tracers=())
    out = (model.get_option("fused_zfft_active"), model.get_option("c2r_strided_active"))
    model.close()
    return out


def _pressure_case(ocn, oracle, arch, size, halo):
    """the fields and the oracle's solve of test_solve_for_pressure_real_transform_path, once per (size, halo)"""
    def make():
        rng = np.random.default_rng(size[2])
        grid = HC.make_grid(ocn, arch, HC.PPP, size, halo)
        g_cpu = HC.make_oracle_grid(oracle, HC.PPP, size, halo)
        U, A = [], []
        for F, loc in ((ocn.XFaceField, "u"), (ocn.YFaceField, "v"), (ocn.ZFaceField, "w")):
            f = F(grid)
            a = np.asfortranarray(rng.standard_normal(f.shape))
            f.set_parent(a)
            ocn.fill_halo_regions(f)
            g_cpu.fill_halo_regions(a, oracle.LOC[loc])
            U.append(f)
            A.append(a)
        s_cpu = oracle.PoissonSolver(g_cpu, 0)
        s_cpu.rhs[...] = g_cpu.source_term(*A)
        p_cpu = g_cpu.zeros(oracle.LOC["c"])
        s_cpu.solve(p_cpu)
        return grid, g_cpu, U, p_cpu
    return _cached(("pressure", size, halo), make)


# N >= H: (10, 6, 7) takes (7, 6, 7) for (7, 7, 7)
PRESSURE_CASES = [(size, HC.clamped(h, size)) for size in ((12, 10, 32), (10, 6, 7)) for h in HC.HALOS]
SOLVER_VARIANTS = [{}, {"real_fft": 0}, {"c2r_strided": 0}, {"fused_zfft": 0}, {"fused_zfft": 0, "c2r_strided": 0}]


@pytest.mark.parametrize("opts", SOLVER_VARIANTS, ids=_tag)
@pytest.mark.parametrize("size,halo", PRESSURE_CASES, ids=["%dx%dx%d-%s" % (*s, HC.halo_id(h)) for s, h in PRESSURE_CASES])
def test_solve_for_pressure_with_every_solver_variant(ocn, oracle, arch, size, halo, opts):
    """solve_for_pressure! as the model runs it, with real_fft, c2r_strided and fused_zfft each at both values, against the oracle at the
    same halo. The strided Z2D plan writes straight into the haloed array at Hx + Px (Hy + Py Hz). The *_active read-backs are asserted both
    ways where the path exists on the grid at (3, 3, 3) (test_pressure_solver_variants_match_the_oracle): the fused z transform needs
    Nz = 2^m; the strided plan is rocFFT's to accept -- where it is on, switching it off reads 0, and no halo may lose a path that
    (3, 3, 3) has without saying so in the read-back"""
    grid, g_cpu, U, p_cpu = _pressure_case(ocn, oracle, arch, size, halo)
    base_paths = _cached(("paths-base", size), lambda: _solver_paths(ocn, HC.make_grid(ocn, arch, HC.PPP, size, HC.BASE)))
    default_paths = _cached(("paths", size, halo), lambda: _solver_paths(ocn, grid))
    print(size, HC.halo_id(halo), "default fused_zfft_active, c2r_strided_active =", default_paths, "at (3, 3, 3):", base_paths)
    assert default_paths[0] == base_paths[0] == (1 if size[2] == 32 else 0), (size, halo, default_paths, base_paths)
    with _options(ocn, opts):
        paths = _solver_paths(ocn, grid)
        solver = ocn.FFTBasedPoissonSolver(grid)
        p = ocn.CenterField(grid)
        p.set_parent(np.full(p.shape, SENTINEL))
        ocn.solve_for_pressure(p, solver, U)
        out = p.parent()
        solver.close()
    if not opts.get("real_fft", 1):
        assert paths == (0, 0), (size, halo, opts, paths)
    else:
        assert paths[0] == (default_paths[0] if opts.get("fused_zfft", 1) else 0), (size, halo, opts, paths)
        if not opts.get("c2r_strided", 1):
            assert paths[1] == 0, (size, halo, opts, paths)
        if opts == {"fused_zfft": 0}:
            assert paths == (0, 1), (size, halo, paths)             # the 3-D strided plan is on when nothing switches it off
    if size == (12, 10, 32) and not opts:
        assert paths == (1, 1), (size, halo, paths)                 # ... and so is the 2-D one beside the fused z transform
    e = rel_err(HC.interior(grid, out), HC.interior(g_cpu, p_cpu))
    print(size, HC.halo_id(halo), _tag(opts), "paths", paths, "rel err", e)
    assert e < 1e-12, (size, halo, opts, e)
    halo_cells = np.ones(out.shape, bool)
    HC.interior(grid, halo_cells)[...] = False
    assert (out[halo_cells] == SENTINEL).all(), (size, halo, opts, "the solve wrote outside the interior")


# ---------------------------------------------------------------------------------------------------------------------
# 4. time steps
# ---------------------------------------------------------------------------------------------------------------------
def _physics(ocn, gid):
    """ppb: the ppb_physics preset of test_time_step_graph_replay_is_bit_identical; bbb: ScalarDiffusivity"""
    if gid == "ppb":
        F = ocn.FieldBoundaryConditions
        return dict(closure=ocn.AnisotropicMinimumDissipation(), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=0.3),
                    boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-3)), "T": F(bottom=ocn.GradientBoundaryCondition(0.1))})
    if gid == "bbb":
        return dict(closure=ocn.ScalarDiffusivity(ν=2e-3, κ={"T": 1e-3, "S": 5e-4}))
    return {}


def _oracle_physics(m_cpu, gid):
    if gid == "ppb":
        m_cpu.set_amd()
        m_cpu.set_seawater_buoyancy()
        m_cpu.set_coriolis(0.3)
        m_cpu.set_bc("u", "top", "flux", -1e-3)
        m_cpu.set_bc("c0", "bottom", "gradient", 0.1)
    if gid == "bbb":
        m_cpu.set_closure(nu=2e-3, kappa=[1e-3, 5e-4])


def _dts(grid, stepper):
    dt = 0.1 * min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.min(grid.Δzᵃᵃᶜ))) / 0.6
    return [dt] * 3 if stepper == "RungeKutta3" else [dt, dt, 0.7 * dt]      # AB2: the second step reads G⁻, the third changes Δt


def _state_of(model):
    return {n: f.parent() for n, f in model.fields().items()} | {"pNHS": model.pressures.pNHS.parent()}


def _values(ocn, grid):
    locs = _locs(ocn)
    return smooth_state({n: grid.nodes(locs[n]) for n in ("u", "v", "w", "T", "S")}, 1234)


def _stepped(ocn, oracle, arch, gid, halo, stepper, opts, nsteps=3, grid=None):
    def make():
        g = grid or _grids(ocn, oracle, arch, gid, halo)[0]
        model = ocn.NonhydrostaticModel(grid=g, advection=ocn.WENO(), tracers=("T", "S"), timestepper=stepper, **_physics(ocn, gid))
        for k, v in opts.items():
            model.set_option(k, v)
        ocn.set_model(model, **_values(ocn, g))
        dts = _dts(g, stepper)
        for n in range(nsteps):
            ocn.time_step(model, dts[n % 3])
        facts = {k: model.get_option(k) for k in ("fuse_substep_active", "halo_fill_folded", "stage1_source_fused", "graph_failures", "graph_captures",
                                                  "graph_replays")}
        state = _state_of(model)
        model.close()
        return state, facts
    return _cached(("stepped", gid, halo, stepper, _tag(opts), nsteps, None if grid is None else grid.size), make)


def _oracle_stepped(ocn, oracle, arch, gid, halo, stepper):
    def make():
        g_gpu, g_cpu = _grids(ocn, oracle, arch, gid, halo)
        m_cpu = oracle.Model(g_cpu, 2)
        _oracle_physics(m_cpu, gid)
        vals = _values(ocn, g_gpu)
        m_cpu.set(**{cn: vals[n] for cn, n in zip(CNAMES, ("u", "v", "w", "T", "S"))})
        for dt in _dts(g_gpu, stepper):
            m_cpu.time_step(dt) if stepper == "RungeKutta3" else m_cpu.time_step_ab2(dt)
        return {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, ("u", "v", "w", "T", "S"))} | {"pNHS": m_cpu.field("p").copy()}
    return _cached(("oracle-stepped", gid, halo, stepper), make)


def _assert_within_1e12_of_the_oracle(ocn, state, ocpu, grid, g_cpu, dt, tag):
    """fields: helpers.rel_err < 1e-12 on the interiors; pNHS: the error model of test_gpu_option_variants.py (p = lap^-1(div u*) / dt carries
    the velocities' round-off times dx / dt on anisotropic cells) -> the worst relative error"""
    locs = _locs(ocn)
    umax = max(np.abs(ocpu[n]).max() for n in ("u", "v", "w"))
    dmax = max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.max(grid.Δzᵃᵃᶜ)))
    worst = 0.0
    for name, a in state.items():
        ia, ib = HC.interior(grid, a, locs[name]), HC.interior(g_cpu, ocpu[name], HC.face_code(ocn, locs[name]))
        assert ia.shape == ib.shape, (tag, name)
        if name == "pNHS":
            pscale = max(np.abs(ib).max(), umax * dmax / dt)
            err = np.max(np.abs(ia - ib))
            worst = max(worst, err / pscale)
            assert err < 1e-12 * pscale, (tag, name, err, pscale)
            continue
        worst = max(worst, rel_err(ia, ib))
        assert rel_err(ia, ib) < 1e-12, (tag, name, rel_err(ia, ib))
    print(tag, "worst rel err vs the oracle", worst)
    return worst


@halos
@pytest.mark.parametrize("stepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("gid", list(HC.GRIDS))
def test_three_steps_match_the_oracle(ocn, oracle, arch, gid, stepper, halo):
    g_gpu, g_cpu = _grids(ocn, oracle, arch, gid, halo)
    state, _facts = _stepped(ocn, oracle, arch, gid, halo, stepper, {})
    _assert_within_1e12_of_the_oracle(ocn, state, _oracle_stepped(ocn, oracle, arch, gid, halo, stepper), g_gpu, g_cpu, _dts(g_gpu, stepper)[-1],
                                      (gid, HC.halo_id(halo), stepper))
    # device against device across halos: printed, not asserted (rocFFT may pick another kernel for other output strides)
    base, _ = _stepped(ocn, oracle, arch, gid, HC.BASE, stepper, {})
    base_grid, locs = _grids(ocn, oracle, arch, gid, HC.BASE)[0], _locs(ocn)
    diff = {n: rel_err(HC.interior(g_gpu, state[n], locs[n]), HC.interior(base_grid, base[n], locs[n])) for n in state}
    print(gid, HC.halo_id(halo), stepper, "difference from the (3, 3, 3) run:", " ".join("%s:%.1e" % kv for kv in diff.items()))


STEP_VARIANTS = [{"fuse_substep": 0}, {"fused_epilogue": 0}, {"epilogue_march": 0}, {"fuse_substep": 0, "fused_epilogue": 0, "epilogue_march": 0}]


@halos
@pytest.mark.parametrize("opts", STEP_VARIANTS, ids=_tag)
@pytest.mark.parametrize("gid", list(HC.GRIDS))
def test_step_variants_are_bit_identical_to_the_default_options(ocn, oracle, arch, gid, opts, halo):
    """fuse_substep, fused_epilogue, epilogue_march at 0 (1 is the default run): 3 RK3 steps, whole parent arrays equal the default options'"""
    ref, ref_facts = _stepped(ocn, oracle, arch, gid, halo, "RungeKutta3", {})
    state, facts = _stepped(ocn, oracle, arch, gid, halo, "RungeKutta3", opts)
    if gid in ("ppp", "ppb"):
        assert ref_facts["fuse_substep_active"] == 1, (gid, halo, ref_facts)
    if "fuse_substep" in opts:
        assert facts["fuse_substep_active"] == 0 and facts["stage1_source_fused"] == 0
    for n in ref:
        assert np.array_equal(state[n], ref[n]), (gid, halo, opts, n, int((state[n] != ref[n]).sum()))


FOLD_SIZES = [(8, 8, 8), (70, 16, 8)]       # the split solver needs Ny = 2^m >= 8 and the fused z transform Nz = 2^m; 8 < 2H at every halo but 3


@halos
@pytest.mark.parametrize("size", FOLD_SIZES, ids=_ids)
def test_folded_pressure_step_against_the_separate_kernels(ocn, oracle, arch, size, halo):
    """triply periodic: the correction kernel writes every periodic image (both sides' images of one cell where N < 2H) and the first
    substep rides in the pressure step. Whole parent arrays, halo images included, equal fused_halo = 0, fuse_substep = 0; every parent
    array is its interior wrapped by the grid's halo"""
    grid = _cached(("fold-grid", size, halo), lambda: HC.make_grid(ocn, arch, HC.PPP, size, halo))
    folded, facts = _stepped(ocn, oracle, arch, "ppp", halo, "RungeKutta3", {}, grid=grid)
    separate, sfacts = _stepped(ocn, oracle, arch, "ppp", halo, "RungeKutta3", {"fused_halo": 0, "fuse_substep": 0}, grid=grid)
    assert (facts["halo_fill_folded"], facts["stage1_source_fused"]) == (1, 1), (size, halo, facts)          # N >= H: no fallback
    assert (sfacts["halo_fill_folded"], sfacts["stage1_source_fused"]) == (0, 0), (size, halo, sfacts)
    for n in separate:
        assert np.array_equal(folded[n], separate[n]), (size, halo, n, int((folded[n] != separate[n]).sum()))
        core = HC.interior(grid, folded[n])
        assert np.abs(core).max() > 0
        assert np.array_equal(folded[n], HC.periodic_pad(grid, core)), (size, halo, n)


@halos
@pytest.mark.parametrize("gid", ["ppp", "ppb", "bbb"])
def test_graph_replay_is_bit_identical(ocn, oracle, arch, gid, halo):
    """use_graph = 1 over 6 steps: the first runs plain, captures and replays follow -- bit-identical to use_graph = 0"""
    ocn.own_stream()
    plain, pfacts = _stepped(ocn, oracle, arch, gid, halo, "RungeKutta3", {"use_graph": 0}, nsteps=6)
    graphed, gfacts = _stepped(ocn, oracle, arch, gid, halo, "RungeKutta3", {"use_graph": 1}, nsteps=6)
    assert pfacts["graph_captures"] == 0 and gfacts["graph_failures"] == 0
    assert gfacts["graph_captures"] >= 1 and gfacts["graph_replays"] >= 1, gfacts
    for n in plain:
        assert np.array_equal(plain[n], graphed[n]), (gid, halo, n)


@halos
@pytest.mark.parametrize("gid", ["ppp", "ppb"])
def test_checkpoint_and_restore_continue_bit_identically(ocn, oracle, arch, tmp_path, gid, halo):
    """test_gpu_parity.py::test_checkpoint_and_restore_continue_bit_identically at other halos: the file holds parent arrays with their halos.
    PPP: bit for bit; PPB (AMD physics): 1e-13, the bound of that test (the tridiagonal solver's singular column is not in the file)"""
    grid = _grids(ocn, oracle, arch, gid, halo)[0]
    locs = _locs(ocn)

    def make():
        return ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), **_physics(ocn, gid))
    model = make()
    ocn.set_model(model, **_values(ocn, grid))
    dt = 0.05 * grid.Δxᶜᵃᵃ
    for _ in range(3):
        ocn.time_step(model, dt)
    path = ocn.write_checkpoint(model, str(tmp_path / f"checkpoint_iteration{model.clock.iteration}"))
    with np.load(path) as file:
        assert tuple(file["NonhydrostaticModel/grid/halo"]) == grid.halo_size
        assert file["NonhydrostaticModel/u/data"].shape == grid.total_size(locs["u"])
        assert file["NonhydrostaticModel/timestepper/Gⁿ/T/data"].shape == grid.total_size(locs["T"])
    for _ in range(3):
        ocn.time_step(model, dt)
    want = {n: f.parent() for n, f in model.fields().items()}
    want_clock = (model.clock.time, model.clock.iteration)
    model.close()
    restored = make()
    ocn.set_from_checkpoint(restored, path)
    assert restored.clock.iteration == 3
    for _ in range(3):
        ocn.time_step(restored, dt)
    assert (restored.clock.time, restored.clock.iteration) == want_clock
    for n, f in restored.fields().items():
        if gid == "ppb":
            assert rel_err(HC.interior(grid, f.parent(), locs[n]), HC.interior(grid, want[n], locs[n])) < 1e-13, n
        else:
            assert np.array_equal(f.parent(), want[n]), n
    restored.close()
    other = HC.make_grid(ocn, arch, HC.GRIDS[gid][0], HC.GRIDS[gid][1], HC.BASE, HC.GRIDS[gid][2])
    other_model = ocn.NonhydrostaticModel(grid=other, tracers=("T", "S"), **_physics(ocn, gid))
    with pytest.raises(ValueError):              # the same grid at another halo: the parent shapes differ
        ocn.set_from_checkpoint(other_model, path)
    other_model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. one smallest case per feature kernel, against its numpy restatement at that halo
# ---------------------------------------------------------------------------------------------------------------------
# The feature tests build their grids through the package object handed to them and take interiors from the grid's own halo, so their
# cases -- fields, programs, positions, and every assertion -- run here unchanged on grids of another halo: halo_cases.AtHalo hands them
# the package (and the oracle) with another default halo. Only cases made of exact operations are taken: every comparison is the `==` (or,
# for sums, the summation bound) of the file it comes from. A grid shorter than the halo in a direction takes N == H there
# (halo_cases.clamped): (70, 9, 6) runs at (7, 7, 6), (70, 5, 13) at (4, 5, 3) and (7, 5, 7).
@pytest.fixture
def at_halo(ocn, oracle, halo):
    return HC.AtHalo(ocn, halo), HC.AtHalo(oracle, halo)


@pytest.fixture(scope="module")
def diagnostics_cases(ocn, oracle, arch):
    import test_gpu_diagnostics as TD
    return {h: {"bpb_stretched": TD.Case(HC.AtHalo(ocn, h), HC.AtHalo(oracle, h), arch, "bpb_stretched")} for h in HC.HALOS}


@halos
@pytest.mark.parametrize("what", ["computed_fields_equal_the_restatement_halos_included", "accumulations_in_the_sequential_order", "extrema_on_all_dims",
                                  "sums_on_all_dims_within_the_summation_bound"])
def test_diagnostics(ocn, diagnostics_cases, what, halo):
    """(70, 37, 9) (Bounded, Periodic, Bounded) stretched: computed fields with their halos, accumulations and extrema `==`, sums within the
    bound of test_gpu_diagnostics.py"""
    import test_gpu_diagnostics as TD
    case = diagnostics_cases[halo]["bpb_stretched"]
    assert case.grid.halo_size == halo and case.oracle_grid.H == halo
    getattr(TD, "test_" + what)(ocn, diagnostics_cases[halo], "bpb_stretched")


@halos
def test_forcing_function_programs(at_halo, arch, halo):
    """the four exact programs of test_exact_programs_equal_the_restatement on grid A, with and without the hoisted tables"""
    import test_gpu_forcing_function as TF
    assert TF._grid(at_halo[0], arch, "A").halo_size == HC.clamped(halo, (70, 9, 6))
    TF.test_exact_programs_equal_the_restatement(at_halo[0], arch, "A")


@halos
@pytest.mark.parametrize("case", [1], ids=["marching-epilogue"])
def test_forcing_function_tendency_identity(at_halo, arch, case, halo):
    import test_gpu_forcing_function as TF
    TF.test_tendency_identity_bitwise(at_halo[0], arch, TF.CASES[case])


@halos
@pytest.mark.parametrize("case", [0, 4], ids=["role-kernel", "marching-epilogue"])
def test_table_relaxation_array_and_multiple_forcings(at_halo, arch, case, halo):
    """G_forced == G_plain + F with table Relaxations, Forcing(array) and a five-term MultipleForcings (test_gpu_forcing.py)"""
    import test_gpu_forcing as TF
    TF.test_tendency_identity_bitwise(at_halo[0], arch, TF.CASES[case])


@halos
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_boundary_function_programs_on_every_side(at_halo, arch, which, halo):
    import test_gpu_boundary_function as TB
    TB.test_exact_programs_equal_the_restatement(at_halo[0], arch, which)


@halos
@pytest.mark.parametrize("name", ["ppb_stretched", "bbb"])
def test_particles_interpolate_and_advect(at_halo, arch, name, halo):
    """the 257 hand-placed positions include the first and the last half cell, where the halo is read, and displacements past the clamps
    1 - H .. N + H of the interpolator's index"""
    import test_gpu_particles as TP
    assert TP._grids(at_halo[0], None, arch, name)[0].halo_size == HC.clamped(halo, TP.CASES[name]["size"])
    TP.test_interpolate_is_the_restatement(at_halo[0], arch, name)
    TP.test_advect_particles_is_the_restatement(at_halo[0], arch, name, 0.5, False)
    TP.test_advect_particles_is_the_restatement(at_halo[0], arch, name, 1.0, True)


@halos
def test_vertically_implicit_solve_and_explicit_part(at_halo, arch, halo):
    import test_gpu_vertically_implicit as TV
    assert TV._grid(at_halo[0], arch, "ppb_stretched").halo_size == HC.clamped(halo, (70, 5, 13))
    TV.test_solve_kernel_is_the_restatement_bit_for_bit(at_halo[0], arch, "ppb_stretched")
    TV.test_explicit_part_is_the_restatement_bit_for_bit(at_halo[0], arch, "ppb_stretched")


@halos
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_vertically_implicit_model(ocn, at_halo, arch, timestepper, halo):
    """the model of test_gpu_vertically_implicit.py::test_model_is_the_orchestrated_yardstick on (70, 5, 13) stretched: 2 steps against the
    orchestrated yardstick at the same halo, with that test's bounds"""
    import test_gpu_vertically_implicit as TV
    size = (70, 5, 13)
    saved = TV.MODEL_GRIDS["ppb_stretched"]
    TV.MODEL_GRIDS["ppb_stretched"] = (size, HC.PPB, True)
    try:
        grid, model, yard = TV._model_pair(at_halo[0], at_halo[1], arch, "ppb_stretched", timestepper)
    finally:
        TV.MODEL_GRIDS["ppb_stretched"] = saved
    assert grid.halo_size == HC.clamped(halo, size) == yard.g.H and grid.size == size
    assert model.get_option("vertically_implicit") == 1
    dt = 0.05 / grid.Nx
    for _ in range(2):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    locs = _locs(ocn)
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    worst = 0.0
    for gn, cn in zip(("u", "v", "w", "T", "S"), yard.names):
        a, b = HC.interior(grid, model.fields()[gn].parent(), locs[gn]), HC.interior(grid, yard.U[cn], locs[gn])
        assert np.all(np.isfinite(a))
        worst = max(worst, rel_err(a, b))
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = HC.interior(grid, model.pressures.pNHS.parent()), HC.interior(grid, yard.p)
    pscale = max(np.abs(b).max(), umax * max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / dt)
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    print("vertically implicit", HC.halo_id(halo), timestepper, "worst rel err", worst, "pNHS", np.max(np.abs(a - b)) / pscale)
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == 2
    model.close()


@halos
@pytest.mark.parametrize("variant,kind,Cb", [("constant", "none", None), ("lilly", "seawater", 0.5)], ids=["Smagorinsky", "Lilly-seawater"])
@pytest.mark.parametrize("name", ["ppb", "bbb"])
def test_smagorinsky_viscosity(ocn, arch, monkeypatch, name, variant, kind, Cb, halo):
    """both eddy-viscosity kernels == the restatement (its grids name halo = (3, 3, 3): rebuilt here with with_halo)"""
    import smagorinsky_reference as SR
    import test_gpu_smagorinsky as TS
    make = SR.make_grid
    monkeypatch.setattr(SR, "make_grid", lambda o, a, n: ocn.grids.with_halo(HC.clamped(halo, SR.GRIDS[n]["size"]), make(o, a, n)))
    assert SR.make_grid(ocn, arch, name).halo_size == HC.clamped(halo, SR.GRIDS[name]["size"])
    TS.test_eddy_viscosity_is_the_restatement_bit_for_bit(ocn, arch, name, variant, kind, Cb)


@halos
@pytest.mark.parametrize("name", ["ppb_stretched", "ppp"])
def test_stokes_drift_kernel(at_halo, arch, name, halo):
    import test_gpu_stokes as TS
    TS.test_raw_kernel_is_the_restatement(at_halo[0], arch, name)


@halos
@pytest.mark.parametrize("name,impl", [("ppb_stretched", 2), ("ppb_stretched", 0), ("bbb", 2)])
def test_background_advective_tendency(ocn, at_halo, arch, name, impl, halo):
    """advecting != advected arrays (the background-field terms): the role kernel's split instantiation and the per-field kernels"""
    import test_gpu_background as TBG
    try:
        TBG.test_raw_entry_point_is_the_restatement(at_halo[0], arch, lambda v: ocn.set_option("tendency_impl", v), name, impl)
    finally:
        ocn.set_option("tendency_impl", 2)


@halos
@pytest.mark.parametrize("name", ["bbb_stretched"])
def test_perturbation_advection_open_boundaries(at_halo, arch, name, halo):
    """the boundary step `==`, the mass-flux integral and correction within the bounds of test_gpu_open_boundary.py"""
    import test_gpu_open_boundary as TO
    TO.test_boundary_step_is_the_restatement_bit_for_bit(at_halo[0], arch, name)
    TO.test_flux_integral_and_correction(at_halo[0], arch, name)


@halos
@pytest.mark.parametrize("name", ["ppb_stretched", "bbb"])
def test_tilted_gravity_kernels(at_halo, arch, name, halo):
    import test_gpu_tilted as TT
    TT.test_cartesian_coriolis_is_the_restatement(at_halo[0], arch, name)
    TT.test_buoyancy_acceleration_is_the_restatement(at_halo[0], arch, name, 2)
    TT.test_tilted_hydrostatic_pressure_is_the_restatement(at_halo[0], arch, name, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the partitioned model inside the library
# ---------------------------------------------------------------------------------------------------------------------
# Virtual ranks as in test_gpu_dist_library.py: R threads sharing the card over the caller-supplied transport (tests/loopback.py), the
# physics presets and the analytic state of that file, the serial oracle of test_gpu_distributed.py on the global grid at the same halo.
DIST_HALOS = ((5, 3, 4), (4, 6, 3))
DIST_CASES = {
    # name: R, size, preset, xbounded, partition, options
    "2-slabs": (2, (32, 12, 10), "stretched", False, None, {}),
    "2-slabs-thick-halos": (2, (32, 12, 10), "stretched", False, None, {"thin_halos": 0}),
    "2-slabs-sync-halos": (2, (32, 12, 10), "stretched", False, None, {"async_halos": 0}),
    "2-slabs-late-exchange": (2, (32, 12, 10), "stretched", False, None, {"early_exchange": 0, "async_halos": 1}),      # interior / strip split, Hx-wide strips
    "2-slabs-strips-of-5": (2, (32, 12, 10), "stretched", False, None, {"early_exchange": 0, "async_halos": 1, "strip_width": 5}),
    # triply periodic: the substructured solves -- x-fastest (the dense strips kernel) and, with the creation key dist_xfast = 0, z-fastest
    "2-slabs-periodic": (2, (32, 16, 8), "periodic", False, None, {}),
    "2-slabs-periodic-zfast": (2, (32, 16, 8), "periodic", False, None, {"dist_xfast": 0}),
    "3-slabs-irregular": (3, (32, 12, 10), "stretched", False, None, {}),                                               # 10 + 10 + 12 columns
    "3-slabs-bounded-x": (3, (25, 8, 6), "periodic", True, None, {}),                                                   # Right-, Fully-, LeftConnected
    "2x2-pencils": (4, (16, 16, 8), "periodic", False, (2, 2), {}),
}


def _run_ranks_at_halo(ocn, arch, halo, R, size, zkind, xbounded, partition, options, nsteps=3):
    from oldoceananigans_jl_amd import _lib, distributed as dist
    from loopback import PointerLoopbackWorld
    from dist_worker import analytic
    from test_gpu_distributed import _bcs, _closure, _tracers_and_buoyancy, _z_and_topology
    world = PointerLoopbackWorld(R, _lib.lib())
    results, errors = [None] * R, []
    dt = 0.1 * (2.0 / size[0]) / 0.6

    def worker(rank):
        try:
            ctx = dist.Distributed.transport(arch, world.collectives(rank), R, rank)
            z, topo = _z_and_topology(ocn, zkind, size[2])
            topo = ((ocn.Bounded if xbounded else topo[0]), topo[1], topo[2])
            grid = dist.DistributedRectilinearGrid(ctx, size=size, x=(0.0, 2.0), y=(0.0, 1.0), z=z, topology=topo, partition=partition, halo=halo)
            model = dist.LibraryDistributedModel(grid=grid, tracers=("T", "S"), boundary_conditions=_bcs(ocn, zkind), closure=_closure(ocn, zkind),
                                                 buoyancy=_tracers_and_buoyancy(ocn, zkind)[1], coriolis=ocn.FPlane(f=0.5) if zkind == "stretched" else None)
            assert grid.local.halo_size == tuple(halo)
            ocn.set_model(model, **{n: analytic(n, *grid.global_nodes(f.loc)) for n, f in model.fields().items()})
            for k, v in options.items():
                model.set_option(k, v)
                assert model.get_option(k) == v
            for _ in range(nsteps):
                ocn.time_step(model, dt)
            out = {n: f.parent() for n, f in model.fields().items()} | {"p": model.pressures.pNHS.parent()}
            results[rank] = (out, ocn.max_abs_divergence(model), model.clock.time, (grid.i_offset, grid.j_offset), grid.local.size)
            model.close()
            ctx.close()
        except BaseException as e:          # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))
            world.barrier_obj.abort()

    import threading
    threads = [threading.Thread(target=worker, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    return results


@pytest.mark.parametrize("halo", DIST_HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("case", list(DIST_CASES))
def test_partitioned_model_matches_the_serial_oracle(ocn, oracle, arch, case, halo):
    """every rank's slab of u, v, w, T, S and p within 1e-12 (of the global maximum, test_gpu_dist_library._compare) of the serial oracle on
    the global grid, the clock `==`; the exchanged halo columns (and rows, for pencils) equal the neighbour's interior bit for bit"""
    from oldoceananigans_jl_amd import _lib
    from test_gpu_distributed import _serial_oracle
    R, size, zkind, xbounded, partition, options = DIST_CASES[case]
    _lib.check(_lib.lib().ocn_own_stream())
    creation = {k: v for k, v in options.items() if k == "dist_xfast"}          # read when the model is built: a library default around the run
    for k, v in creation.items():
        ocn.set_option(k, v)
    try:
        results = _run_ranks_at_halo(ocn, arch, halo, R, size, zkind, xbounded, partition, {k: v for k, v in options.items() if k not in creation})
    finally:
        for k in creation:
            ocn.set_option(k, 1)
    oref, otime = _serial_oracle(ocn, HC.AtHalo(oracle, halo), size, zkind, 3, xbounded, False)
    Hx, Hy, Hz = halo
    assert oref["T"].shape == tuple(n + 2 * h for n, h in zip(size, halo))
    Rx, Ry = partition if partition else (R, 1)
    worst = 0.0
    for r, (out, div, t, (i0, j0), (nxl, nyl, nzl)) in enumerate(results):
        assert div < 5e-8 and t == otime, (case, r, div, t, otime)
        for name, a in out.items():
            nx, ny, nz = a.shape[0] - 2 * Hx, a.shape[1] - 2 * Hy, a.shape[2] - 2 * Hz        # nxl + 1 for the x faces of a LeftConnected rank
            assert (ny, nz) == (nyl, size[2] + (1 if name == "w" and zkind != "periodic" else 0)) and nx - nxl in (0, 1), (case, r, name, a.shape)
            want = oref[name][Hx + i0:Hx + i0 + nx, Hy + j0:Hy + j0 + ny, Hz:Hz + nz]
            err = np.abs(a[Hx:Hx + nx, Hy:Hy + ny, Hz:Hz + nz] - want).max() / np.abs(oref[name]).max()
            worst = max(worst, err)
            assert err <= 1e-12, (case, halo, r, name, err, int(np.isnan(a).sum()))
    print(case, HC.halo_id(halo), "worst err / global max vs the serial oracle", worst)
    # exchanged halos: bit-exact copies of the neighbour's interior cells
    for r, (out, _div, _t, _off, (nxl, nyl, _nzl)) in enumerate(results):
        ix, iy = r // Ry, r % Ry
        for name in ("u", "v", "w", "T", "S"):
            a = out[name]
            core_y, core_z = slice(Hy, Hy + nyl), slice(Hz, Hz + size[2])
            if Rx > 1 and not (xbounded and ix == 0):
                west = results[((ix - 1) % Rx) * Ry + iy]
                b, nw = west[0][name], west[4][0]
                assert np.array_equal(a[:Hx, core_y, core_z], b[nw:nw + Hx, core_y, core_z]), (case, halo, r, name, "west halo")
            if Rx > 1 and not (xbounded and ix == Rx - 1):
                b = results[((ix + 1) % Rx) * Ry + iy][0][name]
                assert np.array_equal(a[Hx + nxl:2 * Hx + nxl, core_y, core_z], b[Hx:2 * Hx, core_y, core_z]), (case, halo, r, name, "east halo")
            if Ry > 1:
                core_x = slice(Hx, Hx + nxl)
                south, north = results[ix * Ry + (iy - 1) % Ry], results[ix * Ry + (iy + 1) % Ry]
                ns = south[4][1]
                assert np.array_equal(a[core_x, :Hy, core_z], south[0][name][core_x, ns:ns + Hy, core_z]), (case, halo, r, name, "south halo")
                assert np.array_equal(a[core_x, Hy + nyl:2 * Hy + nyl, core_z], north[0][name][core_x, Hy:2 * Hy, core_z]), (case, halo, r, name, "north halo")


@pytest.mark.parametrize("halo", DIST_HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("size,zkind", [((32, 16, 8), "periodic"), ((32, 12, 10), "stretched")], ids=["periodic", "stretched"])
def test_self_loop_over_rccl_matches_the_serial_oracle(ocn, oracle, arch, size, zkind, halo):
    """an RCCL communicator of ONE rank that is its own west and east neighbour (test_library_self_loop_over_rccl_equals_single_gpu): the
    partitioned code path through ncclSend / ncclRecv on one card, against the serial oracle at the same halo; the x halos hold bit-exact
    copies of the other side's interior columns"""
    import ctypes as C
    from oldoceananigans_jl_amd import _lib, distributed as dist
    from dist_worker import analytic
    from test_gpu_distributed import _bcs, _closure, _serial_oracle, _tracers_and_buoyancy, _z_and_topology
    _lib.check(_lib.lib().ocn_own_stream())
    uid = C.create_string_buffer(128)
    _lib.check(_lib.lib().ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    z, topo = _z_and_topology(ocn, zkind, size[2])
    grid = dist.DistributedRectilinearGrid(ctx, size=size, x=(0.0, 2.0), y=(0.0, 1.0), z=z, topology=topo, halo=halo)
    model = dist.LibraryDistributedModel(grid=grid, tracers=("T", "S"), boundary_conditions=_bcs(ocn, zkind), closure=_closure(ocn, zkind),
                                         buoyancy=_tracers_and_buoyancy(ocn, zkind)[1], coriolis=ocn.FPlane(f=0.5) if zkind == "stretched" else None)
    assert grid.local.topology[0] is ocn.FullyConnected and grid.local.halo_size == halo
    ocn.set_model(model, **{n: analytic(n, *grid.global_nodes(f.loc)) for n, f in model.fields().items()})
    dt = 0.1 * (2.0 / size[0]) / 0.6
    for _ in range(3):
        ocn.time_step(model, dt)
    assert ocn.max_abs_divergence(model) < 5e-8
    out = {n: f.parent() for n, f in model.fields().items()} | {"p": model.pressures.pNHS.parent()}
    time = model.clock.time
    model.close()
    ctx.close()
    oref, otime = _serial_oracle(ocn, HC.AtHalo(oracle, halo), size, zkind, 3)
    assert time == otime
    Hx, Hy, Hz = halo
    worst = 0.0
    for name, a in out.items():
        assert a.shape == oref[name].shape, name
        core = (slice(Hx, Hx + size[0]), slice(Hy, Hy + size[1]), slice(Hz, a.shape[2] - Hz))
        err = np.abs(a[core] - oref[name][core]).max() / np.abs(oref[name]).max()
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
        if name != "p":
            assert np.array_equal(a[:Hx][:, core[1], core[2]], a[size[0]:size[0] + Hx][:, core[1], core[2]]), (name, "west halo")
            assert np.array_equal(a[Hx + size[0]:][:, core[1], core[2]], a[Hx:2 * Hx][:, core[1], core[2]]), (name, "east halo")
    print("self-loop", zkind, HC.halo_id(halo), "worst err / global max vs the serial oracle", worst)
