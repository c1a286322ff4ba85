"""GPU: the kernel instantiations and host paths that only a NON-DEFAULT tuning option selects (include/ocn_mi355x.h: ocn_set_option;
the values are the table of tests/option_variants.py), each against the oracle or against the per-field kernels that the suite pins to
the oracle -- never HIP against the same HIP kernel alone:

  a. the two flux-sharing tendency kernels at explicit chunk lengths (shorter than the three primed planes, a last chunk of one level,
     longer than the grid), the 64 x 3 tiles, no register z-windows, the XCD tile order, extra dynamic LDS: G bit-identical to the oracle;
  b. the same on KernelParameters ranges against the per-field kernels: equal inside, a sentinel untouched outside;
  c. the RK3 substep riding in those kernels: 3 steps bit-identical to the default options and within 1e-12 of the oracle;
  d. the marching epilogue with every row count and chunk length (AMD, ScalarDiffusivity, SmagorinskyLilly with Pr != 1);
  e. cache_previous_tendencies! as a copy kernel (swap_tendencies = 0), RK3 and AB2;
  f. the pressure solver without the fused z transform, without the strided Z2D plan, on complex transforms, with 8 lines per workgroup;
     the model reports which path its solver took ("fused_zfft_active", "c2r_strided_active") and every case asserts it both ways.

The partitioned solver's variants are preset rows of tests/test_gpu_dist_library.py. No tolerance is new: bit-identity where the suite
asserts it for the default path, helpers.rel_err < 1e-12 after steps, pNHS with the error model of
test_gpu_parity.py::test_tile_edges_of_the_tendency_kernels. Variants that only regroup one IEEE operation sequence (chunks, tiles, rows,
z-windows, tile order, LDS pad) are also bit-identical to the default options after stepping."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import option_variants as V
import smagorinsky_reference as R
from helpers import rel_err, smooth_state, tanh_faces

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
PPP, PPB = ("Periodic", "Periodic", "Periodic"), ("Periodic", "Periodic", "Bounded")
# two x tiles with a ragged second one (70 = 64 + 6, 66 = 64 + 2), two y tiles for 7 rows (12 = 7 + 5, 9 = 7 + 2) and several for 3 rows,
# Nz for several chunks: the grids of test_gpu_parity.py::test_seeded_random_launch_ranges_of_the_flux_sharing_tendency_kernels
GRIDS = {"ppp": (PPP, (70, 12, 20)), "ppb": (PPB, (66, 9, 14))}
CNAMES = ["u", "v", "w", "c0", "c1", "c2"]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_models():
    yield
    for v in _cache.values():
        if hasattr(v, "close"):
            v.close()
    _cache.clear()


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@contextlib.contextmanager
def _options(target, opts):
    """set the options on a model (model.set_option) or as library defaults (the package), restore the table's defaults afterwards"""
    restore = {"tendency_impl": 2, "arithmetic": 0, "fuse_substep": 1}
    try:
        for k, v in opts.items():
            if k in V.VARIANTS and "values" in V.VARIANTS[k]:
                assert v == V.default(k) or v in V.VARIANTS[k]["values"], (k, v)      # the table lists what runs here
            target.set_option(k, v)
        yield
    finally:
        for k in opts:
            target.set_option(k, restore[k] if k in restore else V.default(k))


def _grids(ocn, oracle, arch, gid):
    def make():
        topology, size = GRIDS[gid] if gid in GRIDS else (PPB, gid)
        z = tanh_faces(size[2]) if topology[2] == "Bounded" else (0.0, 1.0)
        g_gpu = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=tuple(getattr(ocn, t) for t in topology))
        g_cpu = oracle.Grid(size, topology=tuple({"Periodic": 0, "Bounded": 1}[t] for t in topology), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
        return g_gpu, g_cpu
    return _cached(("grids", gid), make)


def _tag(opts):
    return "-".join("%s=%d" % kv for kv in opts.items())


def _state_of(model):
    out = {n: f.parent() for n, f in model.fields().items()}
    out["pNHS"] = model.pressures.pNHS.parent()
    return out


def _assert_within_1e12_of_the_oracle(state, ocpu, grid, dt, tag):
    """fields: helpers.rel_err < 1e-12; pNHS: the error model of test_tile_edges_of_the_tendency_kernels (p = lap^-1(div u*) / dt carries the
    velocities' round-off times dx / dt on anisotropic cells)"""
    umax = max(np.abs(ocpu[n]).max() for n in ("u", "v", "w"))
    dmax = max(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.max(grid.Δzᵃᵃᶜ)))
    for name, a in state.items():
        ia, ib = a[3:-3, 3:-3, 3:-3], ocpu[name][3:-3, 3:-3, 3:-3]
        if name == "pNHS":
            pscale = max(np.abs(ib).max(), umax * dmax / dt)
            err = np.max(np.abs(ia - ib))
            print(tag, name, "abs err", err, "bound", 1e-12 * pscale)
            assert err < 1e-12 * pscale, (tag, name, err, pscale)
            continue
        print(tag, name, "rel err", rel_err(ia, ib))
        assert rel_err(ia, ib) < 1e-12, (tag, name, rel_err(ia, ib))


# ---------------------------------------------------------------------------------------------------------------------
# a. tendency kernels against the oracle's G
# ---------------------------------------------------------------------------------------------------------------------
def _tendency_pair(ocn, oracle, arch, gid, ntr):
    """one model per (grid, tracer count) on a seeded random state, set identically on the oracle, WITHOUT the projection (the FFTs differ
    at round-off; tendencies need identical inputs, as in test_tendencies_match_oracle) -> (model, the oracle's G arrays)"""
    def make():
        g_gpu, g_cpu = _grids(ocn, oracle, arch, gid)
        names = ("T", "S", "C3")[:ntr]
        m_gpu = ocn.NonhydrostaticModel(grid=g_gpu, advection=ocn.WENO(), tracers=names)
        m_cpu = oracle.Model(g_cpu, ntr)
        rng = np.random.default_rng(11 + ntr)
        vals = {n: rng.standard_normal(g_gpu.interior_size(f.loc)) for n, f in m_gpu.fields().items()}
        ocn.set_model(m_gpu, enforce_incompressibility=False, **vals)
        m_cpu.set(enforce_incompressibility=False, **{cn: vals[n] for cn, n in zip(CNAMES, m_gpu.fields())})
        m_cpu.update_state(True)
        ref = {n: m_cpu.field("G" + cn).copy() for cn, n in zip(CNAMES, m_gpu.fields())}
        return m_gpu, ref
    m_gpu, ref = _cached(("tend", gid, ntr), make)
    _cache.setdefault(("tend-model", gid, ntr), m_gpu)
    return m_gpu, ref


def _tendency_cases():
    # role kernel: 64 x 7 tiles, both grids have ntile = 2 x 2 = 4 and npair = 4 * ceil(Nz / kchunk) (tile, chunk) pairs, spread over 8 XCD
    # bands of ceil(npair / 8) slots -- slots past npair return early (role_tendency_kernel):
    #   Nz = 20: kchunk 1, 2, 5, 19 -> npair 80, 40, 16, 8 (whole bands); 3, 7 -> 28, 12 (npair % 8 != 0); 20, 21, 64 -> 4 (npair < 8)
    #   Nz = 14: kchunk 1, 7, 13 -> npair 56, 8, 8 (whole bands); 2, 3, 5 -> 28, 20, 12 (npair % 8 != 0); 14, 15, 64 -> 4 (npair < 8)
    cases = []
    for gid, (_topo, size) in GRIDS.items():
        for kc in V.chunk_lengths(size[2]):
            cases.append((gid, 2, 2, {"role_kchunk": kc}))
            cases.append((gid, 2, 1, {"fused_kchunk": kc}))
        for ty in (3, 7):
            for zwin in (0, 1):
                for kc in (0, 3):
                    cases.append((gid, 2, 1, {"fused_ty": ty, "fused_zwin": zwin, "fused_kchunk": kc}))
        cases.append((gid, 2, 1, {"fused_xcd": 1}))
        cases.append((gid, 2, 1, {"fused_xcd": 1, "fused_kchunk": 3}))
        cases.append((gid, 2, 1, {"fused_xcd": 1, "fused_ty": 3, "fused_kchunk": 2}))
        cases.append((gid, 2, 2, {"role_ldspad": 16384}))
        cases.append((gid, 2, 2, {"role_ldspad": 16384, "role_kchunk": 3}))
        for ntr in (0, 3):              # every tracer count is its own instantiation
            cases.append((gid, ntr, 2, {"role_kchunk": 3}))
            cases.append((gid, ntr, 1, {"fused_kchunk": 3}))
            cases.append((gid, ntr, 1, {"fused_ty": 3, "fused_zwin": 1}))
            cases.append((gid, ntr, 1, {"fused_ty": 3, "fused_zwin": 0, "fused_kchunk": 3}))
    return cases


@pytest.mark.parametrize("gid,ntr,impl,opts", _tendency_cases(), ids=lambda v: _tag(v) if isinstance(v, dict) else str(v))
def test_tendency_kernel_variants_are_bit_identical_to_the_oracle(ocn, oracle, arch, gid, ntr, impl, opts):
    """the tendency arrays carry a sentinel: what the kernel wrote equals the oracle bit for bit, and the kernel wrote every value the
    oracle computes (elsewhere the oracle's arrays hold their zeros: halos, the wall faces of w)"""
    m_gpu, ref = _tendency_pair(ocn, oracle, arch, gid, ntr)
    with _options(m_gpu, {"tendency_impl": impl, **opts}):
        assert m_gpu.get_option("fused_tendency_active") == 1
        for n in m_gpu.fields():
            m_gpu.tendency(n).set_parent(np.full(m_gpu.tendency(n).shape, SENTINEL))
        ocn.update_state(m_gpu, True)
        got = {n: m_gpu.tendency(n).parent() for n in m_gpu.fields()}
    for n, a in got.items():
        written = a != SENTINEL
        assert written.sum() >= np.prod(GRIDS[gid][1]) - GRIDS[gid][1][0] * GRIDS[gid][1][1], (n, int(written.sum()))
        assert np.array_equal(a[written], ref[n][written]), (gid, ntr, impl, opts, n, int((a[written] != ref[n][written]).sum()))
        assert not ref[n][~written].any(), (gid, ntr, impl, opts, n, "values the oracle computes were not written", int((ref[n][~written] != 0).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# b. launch ranges against the per-field kernels
# ---------------------------------------------------------------------------------------------------------------------
def _range_fixture(ocn, oracle, arch, gid):
    def make():
        grid, _ = _grids(ocn, oracle, arch, gid)
        mk = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "T": ocn.CenterField, "S": ocn.CenterField}
        F = {n: mk[n](grid) for n in "uvwTS"}
        vals = smooth_state({n: grid.nodes(f.loc) for n, f in F.items()}, 5)
        for n, f in F.items():
            f.set(vals[n])
            ocn.fill_halo_regions(f)
        Nx, Ny, Nz = GRIDS[gid][1]
        ranges = [(5, Nx - 3, 2, Ny - 1, 3, Nz - 2),            # k0 > 1 and k1 < Nz, both x tiles cut
                  (1, Nx, 1, Ny, Nz // 2, Nz // 2),             # a single level
                  (1, Nx, 1, Ny, 1, Nz)]                        # the whole grid
        want = []
        for r in ranges:
            G = {n: mk[n](grid) for n in "uvwTS"}
            for f in G.values():
                f.set_parent(np.full(f.shape, SENTINEL))
            ocn.kernels.compute_Gu(grid, F["u"], F["v"], F["w"], G["u"], kernel_parameters=r)
            ocn.kernels.compute_Gv(grid, F["u"], F["v"], F["w"], G["v"], kernel_parameters=r)
            ocn.kernels.compute_Gw(grid, F["u"], F["v"], F["w"], G["w"], kernel_parameters=r)
            ocn.kernels.compute_Gc(grid, F["u"], F["v"], F["w"], F["T"], G["T"], kernel_parameters=r)
            ocn.kernels.compute_Gc(grid, F["u"], F["v"], F["w"], F["S"], G["S"], kernel_parameters=r)
            want.append({n: f.parent() for n, f in G.items()})
        return grid, mk, F, ranges, want
    return _cached(("ranges", gid), make)


def _range_cases():
    cases = []
    for gid, (_topo, size) in GRIDS.items():
        for kc in (1, 3, size[2] + 1):
            cases.append((gid, 2, {"role_kchunk": kc}))
            cases.append((gid, 1, {"fused_kchunk": kc}))
        cases.append((gid, 1, {"fused_ty": 3}))
        cases.append((gid, 1, {"fused_ty": 3, "fused_zwin": 0, "fused_kchunk": 1}))
    return cases


@pytest.mark.parametrize("gid,impl,opts", _range_cases(), ids=lambda v: _tag(v) if isinstance(v, dict) else str(v))
def test_tendency_kernel_variants_on_launch_ranges(ocn, oracle, arch, gid, impl, opts):
    """KernelParameters launches (the interior / strip ranges of the partitioned update): the flux-sharing kernels against the per-field
    kernels (compute_Gu .. compute_Gc, bit-identical to the oracle) on the same range -- equal inside, the sentinel untouched outside"""
    grid, mk, F, ranges, want = _range_fixture(ocn, oracle, arch, gid)
    for r, ref in zip(ranges, want):
        got = {n: mk[n](grid) for n in "uvwTS"}
        for f in got.values():
            f.set_parent(np.full(f.shape, SENTINEL))
        with _options(ocn, {"tendency_impl": impl, **opts}):
            ocn.kernels.compute_tendencies(grid, F["u"], F["v"], F["w"], [F["T"], F["S"]], got["u"], got["v"], got["w"], [got["T"], got["S"]],
                                           kernel_parameters=r)
        for n in "uvwTS":
            a, b = got[n].parent(), ref[n]
            assert (b != SENTINEL).sum() == (r[1] - r[0] + 1) * (r[3] - r[2] + 1) * (r[5] - r[4] + 1), (n, r)
            assert np.array_equal(a, b), (gid, r, impl, opts, n, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# c. the substep riding along, e. swap_tendencies = 0: stepped states
# ---------------------------------------------------------------------------------------------------------------------
def _dt(grid):
    return 0.1 * min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / 0.6


def _ab2_steps(grid):
    dt = _dt(grid)
    return [dt, dt, 0.7 * dt]          # the second step repeats Δt and is a real AB2 step that reads G⁻; the third changes Δt (an Euler step)


def _stepped_model(ocn, grid, opts, timestepper="RungeKutta3", views=False):
    """a fresh model with the options, smooth_state, 3 steps -> the final parent arrays (and the get_option facts of the run). views: read the
    result through the field objects taken BEFORE the first step"""
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"), timestepper=timestepper)
    with _options(model, opts):
        ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 1234))
        facts = {k: model.get_option(k) for k in ("fuse_substep_active", "substep_in_tendency_kernel", "fused_tendency_active")}
        before = dict(model.fields()) | {"pNHS": model.pressures.pNHS}
        gviews = {"G" + n: model.tendency(n) for n in model.fields()} | {"M" + n: model.tendency(n, previous=True) for n in model.fields()}
        for dt in ([_dt(grid)] * 3 if timestepper == "RungeKutta3" else _ab2_steps(grid)):
            ocn.time_step(model, dt)
        if views:
            state = {n: f.parent() for n, f in before.items()}
            tend = {n: f.parent() for n, f in gviews.items()}
        else:
            state = _state_of(model)
            tend = {"G" + n: model.tendency(n).parent() for n in model.fields()} | {"M" + n: model.tendency(n, previous=True).parent() for n in model.fields()}
    model.close()
    return state, tend, facts


def _oracle_steps(ocn, oracle, arch, gid, timestepper="RungeKutta3"):
    def make():
        g_gpu, g_cpu = _grids(ocn, oracle, arch, gid)
        m_cpu = oracle.Model(g_cpu, 2)
        locs = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face),
                "T": (ocn.Center,) * 3, "S": (ocn.Center,) * 3}
        vals = smooth_state({n: g_gpu.nodes(loc) for n, loc in locs.items()}, 1234)
        m_cpu.set(**{cn: vals[n] for cn, n in zip(CNAMES, locs)})
        if timestepper == "RungeKutta3":
            for _ in range(3):
                m_cpu.time_step(_dt(g_gpu))
        else:
            for dt in _ab2_steps(g_gpu):
                m_cpu.time_step_ab2(dt)
        out = {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, locs)}
        out["pNHS"] = m_cpu.field("p").copy()
        return out
    return _cached(("oracle-steps", gid, timestepper), make)


def _default_steps(ocn, oracle, arch, gid, opts=None, timestepper="RungeKutta3"):
    return _cached(("default-steps", gid, timestepper, _tag(opts or {})),
                   lambda: _stepped_model(ocn, _grids(ocn, oracle, arch, gid)[0], opts or {}, timestepper))


def _substep_cases():
    cases = []
    for gid, (_topo, size) in GRIDS.items():
        cases += [(gid, {"role_kchunk": kc}) for kc in (1, 3, size[2] - 1)]
        cases += [(gid, {"tendency_impl": 1, "fused_kchunk": kc}) for kc in (1, 3)]
        cases += [(gid, {"tendency_impl": 1, "fused_ty": 3}), (gid, {"tendency_impl": 1, "fused_ty": 3, "fused_zwin": 0, "fused_kchunk": 3})]
    return cases


@pytest.mark.parametrize("gid,opts", _substep_cases(), ids=lambda v: _tag(v) if isinstance(v, dict) else str(v))
def test_the_substep_rides_along_at_every_chunking(ocn, oracle, arch, gid, opts):
    """RK3 stages 2 and 3 take their substep inside the tendency kernel (fuse_substep = 1, the default): the chunk seams re-prime and close
    gmnn / the previous tendency like the fluxes. 3 steps: bit-identical to the default options, within 1e-12 of the oracle"""
    grid = _grids(ocn, oracle, arch, gid)[0]
    ref, _tend, ref_facts = _default_steps(ocn, oracle, arch, gid)
    assert ref_facts == {"fuse_substep_active": 1, "substep_in_tendency_kernel": 1, "fused_tendency_active": 1}
    state, _tend, facts = _stepped_model(ocn, grid, opts)
    assert facts == ref_facts, (opts, facts)
    for n in ref:
        assert np.array_equal(state[n], ref[n]), (gid, opts, n, int((state[n] != ref[n]).sum()))
    _assert_within_1e12_of_the_oracle(state, _oracle_steps(ocn, oracle, arch, gid), grid, _dt(grid), (gid, _tag(opts)))


@pytest.mark.parametrize("gid", list(GRIDS))
def test_chunking_does_not_change_the_bits_of_the_contracted_kernel(ocn, oracle, arch, gid):
    """arithmetic = 1 (the role kernel's contracted WENO flux) at chunk lengths 1, 3 and Nz - 1 against arithmetic = 1 at the automatic
    chunking, bitwise, substep riding along; its distance from the oracle is the business of test_gpu_arithmetic_mode.py"""
    grid = _grids(ocn, oracle, arch, gid)[0]
    ref, _tend, facts = _default_steps(ocn, oracle, arch, gid, {"arithmetic": 1})
    assert facts["substep_in_tendency_kernel"] == 1
    plain = _default_steps(ocn, oracle, arch, gid)[0]
    assert any(not np.array_equal(ref[n], plain[n]) for n in ref)           # the contracted flux ran
    for kc in (1, 3, GRIDS[gid][1][2] - 1):
        state, _tend, f = _stepped_model(ocn, grid, {"arithmetic": 1, "role_kchunk": kc})
        assert f == facts
        for n in ref:
            assert np.array_equal(state[n], ref[n]), (gid, kc, n)


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("gid", list(GRIDS))
def test_caching_the_previous_tendencies_by_copy(ocn, oracle, arch, gid, timestepper):
    """swap_tendencies = 0: cache_previous_tendencies! is a copy kernel and the substep cannot ride along (fuse_substep_active reads 0).
    3 steps (AB2: Δt, Δt, 0.7 Δt -- its second step reads G⁻): fields, pNHS, Gⁿ and G⁻ bit-identical to swap_tendencies = 1 with
    fuse_substep = 0, read through the field objects taken before the first step; within 1e-12 of the oracle"""
    grid = _grids(ocn, oracle, arch, gid)[0]
    ref, ref_tend, ref_facts = _default_steps(ocn, oracle, arch, gid, {"fuse_substep": 0}, timestepper)
    state, tend, facts = _stepped_model(ocn, grid, {"swap_tendencies": 0}, timestepper, views=True)
    assert facts["fuse_substep_active"] == 0 and facts["substep_in_tendency_kernel"] == 0 and ref_facts["fuse_substep_active"] == 0
    if timestepper == "RungeKutta3":
        assert _default_steps(ocn, oracle, arch, gid)[2]["fuse_substep_active"] == 1          # ... and the default has it
    for n in ref:
        assert np.array_equal(state[n], ref[n]), (gid, timestepper, n)
    for n in ref_tend:
        assert np.array_equal(tend[n], ref_tend[n]), (gid, timestepper, n)
        assert np.abs(tend[n]).max() > 0, n
    _assert_within_1e12_of_the_oracle(state, _oracle_steps(ocn, oracle, arch, gid, timestepper), grid,
                                      _dt(grid) if timestepper == "RungeKutta3" else _ab2_steps(grid)[-1], (gid, timestepper))


# ---------------------------------------------------------------------------------------------------------------------
# d. the marching epilogue
# ---------------------------------------------------------------------------------------------------------------------
# three 62-column blocks (OCN_EPI_MARCH_COLS) with a ragged last one (125 = 62 + 62 + 1), Ny = 9 a multiple of no row count in {2, 4, 8}
# and ragged for 1 .. 8 rows except 1, 3; 12 levels: chunk lengths 1, 2, 3 (shorter than the look-ahead), 12 (one chunk), 13 (longer)
EPI_SIZE = (125, 9, 12)
ALPHA, BETA, RATE = 2e-4, 8e-4, 2.5e-3
EPI_VARIANTS = [{"epilogue_rows": r} for r in (1, 2, 3, 8)] + [{"epilogue_kchunk": k} for k in (1, 2, 3, 12, 13)] + [{"epilogue_rows": 3, "epilogue_kchunk": 1}]


def _epilogue_model(ocn, grid, closure):
    """the physics of test_ocean_wind_mixing_and_convection_physics_matches_oracle plus an f-plane: closure, FPlane, linear SeawaterBuoyancy,
    wind stress, heat flux, bottom gradient and the field-dependent evaporation flux"""
    F = ocn.FieldBoundaryConditions
    bcs = {"u": F(top=ocn.FluxBoundaryCondition(-1e-3)),
           "T": F(top=ocn.FluxBoundaryCondition(4e-3), bottom=ocn.GradientBoundaryCondition(0.01)),
           "S": F(top=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(b=-RATE), field_dependencies="S", parameters=RATE))}
    cl = {"amd": lambda: ocn.AnisotropicMinimumDissipation(), "scalar": lambda: ocn.ScalarDiffusivity(ν=2e-3, κ={"T": 1e-3, "S": 5e-4})}[closure]()
    return ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=cl, coriolis=ocn.FPlane(f=0.3), boundary_conditions=bcs,
                                   buoyancy=ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=ALPHA, haline_contraction=BETA)))


def _epilogue_oracle(oracle, g_cpu, closure):
    m_cpu = oracle.Model(g_cpu, 2)
    if closure == "amd":
        m_cpu.set_amd()
    else:
        m_cpu.set_closure(nu=2e-3, kappa=[1e-3, 5e-4])
    m_cpu.set_coriolis(0.3)
    m_cpu.set_seawater_buoyancy(alpha=ALPHA, beta=BETA)
    m_cpu.set_bc("u", "top", "flux", -1e-3)
    m_cpu.set_bc("c0", "top", "flux", 4e-3)
    m_cpu.set_bc("c0", "bottom", "gradient", 0.01)
    m_cpu.set_linear_flux_bc("c1", "top", 0.0, -RATE, "c1")
    return m_cpu


def _epi_dt(grid):
    return 0.1 * min(grid.Δxᶜᵃᵃ, float(np.min(grid.Δzᵃᵃᶜ))) / 0.6


def _epilogue_reference(ocn, oracle, arch, closure):
    """per closure, once: the oracle's tendencies on a seeded random state (no projection), the oracle after 3 steps from smooth_state, the
    default-option run of the product"""
    def make():
        g_gpu, g_cpu = _grids(ocn, oracle, arch, EPI_SIZE)
        rng = np.random.default_rng(8)
        m = _epilogue_model(ocn, g_gpu, closure)
        rand = {n: rng.standard_normal(g_gpu.interior_size(f.loc)) for n, f in m.fields().items()}
        smooth = smooth_state({n: g_gpu.nodes(f.loc) for n, f in m.fields().items()}, 1234)
        m.close()
        m_cpu = _epilogue_oracle(oracle, g_cpu, closure)
        m_cpu.set(enforce_incompressibility=False, **{cn: rand[n] for cn, n in zip(CNAMES, "uvwTS")})
        m_cpu.update_state(True)
        G = {n: m_cpu.field("G" + cn).copy() for cn, n in zip(CNAMES, "uvwTS")}
        m_cpu = _epilogue_oracle(oracle, g_cpu, closure)
        m_cpu.set(**{cn: smooth[n] for cn, n in zip(CNAMES, "uvwTS")})
        for _ in range(3):
            m_cpu.time_step(_epi_dt(g_gpu))
        stepped = {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, "uvwTS")} | {"pNHS": m_cpu.field("p").copy()}
        return rand, smooth, G, stepped
    return _cached(("epi", closure), make)


def _epilogue_run(ocn, grid, make_model, opts, rand, smooth):
    """-> tendencies on the random state, the state after 3 steps from the smooth one, with the options"""
    model = make_model()
    with _options(model, opts):
        assert model.get_option("epilogue_march") == 1 and model.get_option("fuse_substep_active") == 1
        assert model.get_option("substep_in_tendency_kernel") == 0           # the substep rides in the epilogue march
        ocn.set_model(model, enforce_incompressibility=False, **rand)
        ocn.update_state(model, True)
        G = {n: model.tendency(n).parent() for n in model.fields()}
        try:
            nu = model.diffusivity_fields.νₑ.parent()
        except AttributeError:          # a closure without an eddy-viscosity field
            nu = None
        P = {n: f.parent() for n, f in model.fields().items()}
        ocn.set_model(model, **smooth)
        for _ in range(3):
            ocn.time_step(model, _epi_dt(grid))
        state = _state_of(model)
    model.close()
    return G, state, nu, P


@pytest.mark.parametrize("closure,opts", [("amd", o) for o in EPI_VARIANTS] + [("scalar", {"epilogue_rows": 3, "epilogue_kchunk": 1})],
                         ids=lambda v: _tag(v) if isinstance(v, dict) else str(v))
def test_marching_epilogue_variants_match_the_oracle(ocn, oracle, arch, closure, opts):
    """tendency_epilogue_march_kernel with 1 .. 8 rows per block and explicit chunk lengths (AMD: array coefficients; ScalarDiffusivity: the
    CLO = 1 instantiation): tendencies bit-identical to the oracle, 3 steps bit-identical to the default options and within 1e-12 of the oracle"""
    grid = _grids(ocn, oracle, arch, EPI_SIZE)[0]
    rand, smooth, G_cpu, stepped = _epilogue_reference(ocn, oracle, arch, closure)
    make = lambda: _epilogue_model(ocn, grid, closure)          # noqa: E731
    default = _cached(("epi-default", closure), lambda: _epilogue_run(ocn, grid, make, {}, rand, smooth))
    G, state, _nu, _P = _epilogue_run(ocn, grid, make, opts, rand, smooth)
    for n in G:
        assert np.array_equal(default[0][n], G_cpu[n]), ("default options", closure, n)
        assert np.array_equal(G[n], G_cpu[n]), (closure, opts, n, int((G[n] != G_cpu[n]).sum()))
    for n in state:
        assert np.array_equal(state[n], default[1][n]), (closure, opts, n)
    # (the cells are strongly anisotropic, 125 x 9 x 12 on the unit cube: pNHS takes the error model of the tile-edge test like everywhere here)
    _assert_within_1e12_of_the_oracle(state, stepped, grid, _epi_dt(grid), (closure, _tag(opts)))


def _smagorinsky_model(ocn, grid):
    """the physics of test_gpu_smagorinsky._physics_model with Pr = {T: 1, S: 3} (the PRD instantiation of the epilogue march)"""
    F = ocn.FieldBoundaryConditions
    return ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=ocn.SmagorinskyLilly(Pr={"T": 1.0, "S": 3.0}), coriolis=ocn.FPlane(f=0.3),
                                   buoyancy=ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=R.ALPHA, haline_contraction=R.BETA),
                                                                 gravitational_acceleration=R.GRAV),
                                   boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-3)), "T": F(top=ocn.FluxBoundaryCondition(4e-3))})


def test_marching_epilogue_variant_with_smagorinsky_lilly(ocn, oracle, arch):
    """SmagorinskyLilly with a Prandtl number per tracer at epilogue_rows = 3, epilogue_kchunk = 1, against the references of
    tests/test_gpu_smagorinsky.py: Gⁿ == ((advective G - Coriolis) - hydrostatic gradient) - closure term assembled from the oracle's pieces
    with the model's νₑ (== the numpy restatement), the Pr = 3 tracer with the restatement's ∇·q; 3 steps bit-identical to the default
    options and to every fused path switched off (test_step_paths_agree_bitwise's reference)"""
    from test_gpu_smagorinsky import ORO_LOC, _oracle_closure_term
    grid, g = _grids(ocn, oracle, arch, EPI_SIZE)
    make = lambda: _smagorinsky_model(ocn, grid)          # noqa: E731
    m = make()
    locs = {n: f.loc for n, f in m.fields().items()}
    m.close()
    rand, _names = R.case_values(grid, "seawater")          # smooth_state plus the stratification that puts cells into each regime of ς
    smooth = dict(rand)
    opts = {"epilogue_rows": 3, "epilogue_kchunk": 1}
    G, state, nu_h, P = _epilogue_run(ocn, grid, make, opts, rand, smooth)
    G_def, state_def, _nu, _P = _epilogue_run(ocn, grid, make, {}, rand, smooth)
    # the reference: the oracle's pieces (test_model_tendencies_are_the_oracle_pieces)
    mt = R.Metrics(grid)
    want = ocn.CenterField(grid)
    want.set(R.viscosity(mt, P["u"], P["v"], P["w"], 0.16, Cb=1.0, buoyancy=("seawater", P["T"], P["S"], R.GRAV, R.ALPHA, R.BETA)))
    ocn.fill_halo_regions([want])
    assert np.array_equal(nu_h, want.parent()) and nu_h.max() > 0
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)          # noqa: E731
    u, v, w, T, S = [np.asfortranarray(P[n]) for n in ("u", "v", "w", "T", "S")]
    ref = {}
    for n in ("u", "v", "w"):
        ref[n] = g.zeros(ORO_LOC[n])
        g.compute_G(n, u, v, w, ref[n])
    for n, c in (("T", T), ("S", S)):
        ref[n] = g.zeros((0, 0, 0))
        g.compute_G("c", u, v, w, ref[n], c=c)
    L = oracle.lib()
    L.oro_add_fplane_coriolis.argtypes = [C.c_void_p, C.c_double, dp, dp, dp, dp]
    L.oro_add_fplane_coriolis(g.handle, 0.3, ptr(u), ptr(v), ptr(ref["u"]), ptr(ref["v"]))
    pHY = g.zeros((0, 0, 0))
    L.oro_update_hydrostatic_pressure(g.handle, 2, ptr(T), ptr(S), R.GRAV, R.ALPHA, R.BETA, ptr(pHY))
    L.oro_add_hydrostatic_pressure_gradient(g.handle, ptr(pHY), ptr(ref["u"]), ptr(ref["v"]))
    for which, n in enumerate(("u", "v", "w")):
        ref[n] = _oracle_closure_term(oracle, g, which, P, None, nu_h, ref[n])
    ref["T"] = _oracle_closure_term(oracle, g, 3, P, T, nu_h, ref["T"])
    core = (slice(3, 3 + grid.Nx), slice(3, 3 + grid.Ny), slice(3, 3 + grid.Nz))
    ref["S"][core] = (ref["S"][core] - R.div_q(mt, P["S"], nu_h, 3.0)) + 0.0
    for n in ("u", "v", "w", "T", "S"):
        sl = tuple(slice(3, 3 + k) for k in grid.interior_size(locs[n]))
        assert np.array_equal(G_def[n][sl], ref[n][sl]), ("default options", n)
        assert np.array_equal(G[n][sl], ref[n][sl]), (opts, n, int((G[n][sl] != ref[n][sl]).sum()))
    plain = {k: 0 for k in ("fused_epilogue", "epilogue_march", "smag_march", "fuse_substep")}
    model = make()
    for k, val in plain.items():
        model.set_option(k, val)
    ocn.set_model(model, **smooth)
    for _ in range(3):
        ocn.time_step(model, _epi_dt(grid))
    state_plain = _state_of(model)
    model.close()
    for n in state:
        assert np.isfinite(state[n]).all()
        assert np.array_equal(state[n], state_def[n]), (opts, n)
        assert np.array_equal(state[n], state_plain[n]), ("every fused path off", n)


# ---------------------------------------------------------------------------------------------------------------------
# f. the single-GPU pressure solver
# ---------------------------------------------------------------------------------------------------------------------
def _solver_paths(ocn, grid):
    """which path a model's solver takes on this grid with the library defaults of the moment"""
    model = ocn.NonhydrostaticModel(grid=grid, tracers=())
    out = (model.get_option("fused_zfft_active"), model.get_option("c2r_strided_active"))
    assert model.get_option("dist_yline_active") == 0 and model.get_option("dist_xline_group_active") == 0         # a single-GPU model
    model.close()
    return out


def _pressure_case(ocn, oracle, arch, size):
    """the fields and the oracle's solve of test_solve_for_pressure_real_transform_path, once per size"""
    def make():
        rng = np.random.default_rng(size[2])
        grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
        g_cpu = oracle.Grid(size)
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
        return grid, U, p_cpu, _solver_paths(ocn, grid)
    return _cached(("pressure", size), make)


def _solve_with(ocn, grid, U, opts):
    with _options(ocn, opts):
        paths = _solver_paths(ocn, grid)
        solver = ocn.FFTBasedPoissonSolver(grid)
        p = ocn.CenterField(grid)
        p.set_parent(np.full(p.shape, SENTINEL))
        ocn.solve_for_pressure(p, solver, U)
        out = p.parent()
        solver.close()
    return out, paths


SOLVER_VARIANTS = [{"fused_zfft": 0}, {"c2r_strided": 0}, {"fused_zfft": 0, "c2r_strided": 0}]


@pytest.mark.parametrize("real_fft", [1, 0])
@pytest.mark.parametrize("opts", SOLVER_VARIANTS, ids=_tag)
@pytest.mark.parametrize("size", [(16, 16, 16), (12, 10, 32)])
def test_pressure_solver_variants_match_the_oracle(ocn, oracle, arch, size, opts, real_fft):
    """solve_for_pressure! with the unfused z transform (3-D rocFFT plans + divide kernel), with Z2D into a dense array plus a copy, with
    both, on real and on complex transforms, against the oracle at the bound of test_solve_for_pressure_real_transform_path. The model
    says which path its solver took: a switched-off path reads 0 and the same path reads 1 with the switch on, on the same grid -- so the
    variant IS another path. On complex transforms (real_fft = 0) neither stage exists and both read 0.
    The strided Z2D plan is conditional on rocFFT: it accepts the embedded 3-D plan at both sizes and the embedded 2-D plan (the one beside
    the fused z transform) at 12 x 10, but refuses the 2-D plan at 16 x 16 (measured on the MI355X: also at 8 x 8, 32 x 32, 64 x 64 -- the
    solver then keeps the dense plan, silently before "c2r_strided_active" existed). So at (16, 16, 16) the switch is pinned in its 3-D
    form -- "on" is the fused_zfft = 0 solver -- and (12, 10, 32) pins both forms; what the default reads at 16 x 16 is printed, not asserted."""
    grid, U, p_cpu, default_paths = _pressure_case(ocn, oracle, arch, size)
    print(size, "default options: fused_zfft_active, c2r_strided_active =", default_paths)
    assert default_paths[0] == 1, (size, default_paths)
    unfused_paths = _cached(("unfused-paths", size), lambda: _solve_with(ocn, grid, U, {"fused_zfft": 0})[1])
    assert unfused_paths == (0, 1), (size, unfused_paths)                       # the 3-D strided plan is on when nothing switches it off
    if size == (12, 10, 32):
        assert default_paths == (1, 1), (size, default_paths)                   # ... and so is the 2-D one
    p, paths = _solve_with(ocn, grid, U, {**opts, "real_fft": real_fft})
    want = (opts.get("fused_zfft", 1), opts.get("c2r_strided", 1)) if real_fft else (0, 0)
    assert paths == want, (size, opts, real_fft, paths)
    e = rel_err(p[3:-3, 3:-3, 3:-3], p_cpu[3:-3, 3:-3, 3:-3])
    print(size, _tag(opts), "real_fft", real_fft, "rel err", e)
    assert e < 1e-12, (size, opts, real_fft, e)


def test_line_transforms_with_eight_lines_per_workgroup(ocn, oracle, arch):
    """line_zl512 = 8: zline_solve_kernel<8> on 512-point lines (64 KB of LDS per workgroup) at (4, 4, 512) -- fewer lines than a workgroup
    takes -- against the oracle; the choice is unconditional (line_zl), the fused z transform is on either way"""
    size = (4, 4, 512)
    grid, U, p_cpu, default_paths = _pressure_case(ocn, oracle, arch, size)
    assert default_paths[0] == 1
    p, paths = _solve_with(ocn, grid, U, {"line_zl512": 8})
    assert paths[0] == 1
    e = rel_err(p[3:-3, 3:-3, 3:-3], p_cpu[3:-3, 3:-3, 3:-3])
    print(size, "line_zl512 = 8 rel err", e)
    assert e < 1e-12, e
    p4, _ = _solve_with(ocn, grid, U, {})
    assert rel_err(p4[3:-3, 3:-3, 3:-3], p_cpu[3:-3, 3:-3, 3:-3]) < 1e-12


@pytest.mark.parametrize("opts", SOLVER_VARIANTS + [{"real_fft": 0}], ids=_tag)
def test_model_steps_with_pressure_solver_variants(ocn, oracle, arch, opts):
    """3 RK3 steps at (16, 16, 16) with each solver variant (creation keys set before the model is built): within 1e-12 of the oracle"""
    size = (16, 16, 16)
    g_cpu = oracle.Grid(size)

    def reference():
        grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
        m_cpu = oracle.Model(g_cpu, 2)
        locs = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face),
                "T": (ocn.Center,) * 3, "S": (ocn.Center,) * 3}
        vals = smooth_state({n: grid.nodes(loc) for n, loc in locs.items()}, 1234)
        m_cpu.set(**{cn: vals[n] for cn, n in zip(CNAMES, locs)})
        for _ in range(3):
            m_cpu.time_step(_dt(grid))
        return grid, vals, {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, locs)} | {"pNHS": m_cpu.field("p").copy()}
    grid, vals, ref = _cached(("solver-steps",), reference)
    with _options(ocn, opts):
        model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    want = (opts.get("fused_zfft", 1), opts.get("c2r_strided", 1)) if opts.get("real_fft", 1) else (0, 0)
    assert (model.get_option("fused_zfft_active"), model.get_option("c2r_strided_active")) == want, opts
    ocn.set_model(model, **vals)
    for _ in range(3):
        ocn.time_step(model, _dt(grid))
    state = _state_of(model)
    model.close()
    for n in state:
        e = rel_err(state[n][3:-3, 3:-3, 3:-3], ref[n][3:-3, 3:-3, 3:-3])
        print(_tag(opts), n, "rel err", e)
        assert e < 1e-12, (opts, n, e)
