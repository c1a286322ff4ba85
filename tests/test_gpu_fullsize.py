"""GPU: BASELINE.json's full sizes. HIP against the oracle field by field after one RK3 step (the oracle takes seconds per step here):
configs[1] on the survey's own state, configs[2] and the configs[4] physics on the configs[2] grid. Around them, size-independent
properties the algorithm guarantees:
  * the fused flux-sharing tendency kernel and the per-field kernels (the reference's launch structure, already compared bit for
    bit with the oracle at small sizes) agree bit for bit on all 5 x 256^3 tendencies;
  * halos equal the wrapped interior exactly after a fill;
  * the projection leaves max|div u| at round-off (test/test_time_stepping.jl:124-160 bound 5e-8) and the discrete Laplacian of the
    pressure equals the divergence of the predictor velocities (test/dependencies_for_poisson_solvers.jl:111-129);
  * tracer means are conserved (test/test_time_stepping.jl:165-199);
  * the fused RK3 substep path and the separate-kernel path give identical bits after full time-steps."""
import numpy as np
import pytest

from helpers import smooth_state

pytestmark = pytest.mark.gpu
N = 256


@pytest.fixture(scope="module")
def big(ocn, arch):
    grid = ocn.RectilinearGrid(arch, size=(N, N, N), extent=(1, 1, 1))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=1234))
    yield grid, model
    model.close()


def test_fused_and_per_field_tendencies_agree_bitwise_at_256(ocn, big):
    grid, model = big
    out = []
    for impl in (0, 1, 2):
        model.set_option("tendency_impl", impl)
        ocn.update_state(model, True)
        out.append([model.tendency(n).parent()[3:-3, 3:-3, 3:-3].copy() for n in model.fields()])
    for a, b, c, n in zip(out[0], out[1], out[2], model.fields()):
        assert np.array_equal(a, b) and np.array_equal(a, c), n
        assert np.isfinite(a).all() and np.abs(a).max() > 0


def test_halos_equal_wrapped_interior_at_256(ocn, big):
    grid, model = big
    f = model.fields()["T"]
    rng = np.random.default_rng(0)
    f.set_parent(rng.standard_normal(f.shape))
    ocn.fill_halo_regions(f)
    a = f.parent()
    idx = [np.r_[N:N + 3, 3:3 + N, 3:6] for _ in range(3)]          # wrapped source index of every parent index
    sample = rng.integers(0, N + 6, size=(20000, 3))
    assert np.array_equal(a[sample[:, 0], sample[:, 1], sample[:, 2]],
                          a[idx[0][sample[:, 0]], idx[1][sample[:, 1]], idx[2][sample[:, 2]]])
    ocn.set_model(model, **smooth_state({n: grid.nodes(g.loc) for n, g in model.fields().items()}, seed=1234))


def test_projection_and_conservation_at_256(ocn, big):
    grid, model = big
    dt = 0.1 / N / 0.6
    interior = (slice(3, -3),) * 3
    mean0 = {n: model.fields()[n].parent()[interior].mean() for n in ("T", "S")}
    for _ in range(3):
        ocn.time_step(model, dt)
    assert ocn.max_abs_divergence(model) < 5e-8
    for n in ("T", "S"):
        assert abs(model.fields()[n].parent()[interior].mean() - mean0[n]) < 1e-13 * max(1.0, abs(mean0[n]))
    # ∇²p = ∇·u* / Δt on the last stage: re-derive u* = u + Δt_stage ∇p and compare its divergence with the Laplacian of p
    p = model.pressures.pNHS.parent()
    ocn.fill_halo_regions(model.pressures.pNHS)
    p = model.pressures.pNHS.parent()
    h = 1.0 / N
    c = p[interior]
    lap = ((p[4:-2, 3:-3, 3:-3] - 2 * c + p[2:-4, 3:-3, 3:-3]) + (p[3:-3, 4:-2, 3:-3] - 2 * c + p[3:-3, 2:-4, 3:-3]) +
           (p[3:-3, 3:-3, 4:-2] - 2 * c + p[3:-3, 3:-3, 2:-4])) / h ** 2
    assert np.isfinite(lap).all()
    assert abs(lap.mean()) < 1e-9 * np.abs(lap).max()              # a periodic Laplacian has zero mean: the solve removed the null mode


def test_fused_substep_equals_separate_kernels_at_256(ocn, arch, big):
    grid, model = big
    dt = 0.1 / N / 0.6
    start = {n: f.parent() for n, f in model.fields().items()}
    results = []
    for fuse in (1, 0):
        for n, f in model.fields().items():
            f.set_parent(start[n])
        ocn.update_state(model, True)
        model.set_option("fuse_substep", fuse)
        it0 = model.clock.iteration
        for _ in range(2):
            ocn.time_step(model, dt)
        assert model.clock.iteration == it0 + 2
        results.append({n: f.parent()[3:-3, 3:-3, 3:-3].copy() for n, f in model.fields().items()})
    model.set_option("fuse_substep", 1)
    for n in results[0]:
        assert np.array_equal(results[0][n], results[1][n]), n


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE.json configs[2]: 256 x 256 x 128 (Periodic, Periodic, Bounded), tanh-stretched z, Fourier-tridiagonal solver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_ppb(ocn, arch):
    from helpers import tanh_faces
    grid = ocn.RectilinearGrid(arch, size=(N, N, N // 2), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N // 2),
                               topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=1234))
    yield grid, model
    model.close()


def test_tendency_kernels_agree_bitwise_at_config2(ocn, big_ppb):
    """per-field kernels (the reference's launch structure, bit-identical to the oracle at small sizes), the all-fields kernel and
    the role kernel on the stretched Bounded-z grid: the wall fallbacks (WENO{2}, UpwindBiased{1}, Centered{1} within 3 cells of
    the bottom and the top) and the exclude_periphery mask of Gw ride in every plane of the z-march"""
    grid, model = big_ppb
    out = []
    for impl in (0, 1, 2):
        model.set_option("tendency_impl", impl)
        for n in model.fields():
            model.tendency(n).set_parent(np.zeros(model.tendency(n).shape))
        ocn.update_state(model, True)
        out.append([model.tendency(n).parent() for n in model.fields()])
    for a, b, c, n in zip(out[0], out[1], out[2], model.fields()):
        assert np.array_equal(a, b) and np.array_equal(a, c), n        # whole parent arrays: nothing outside the interior is written
        assert np.isfinite(a).all() and np.abs(a).max() > 0
    gw = out[2][2]
    assert not gw[3:-3, 3:-3, 3].any() and not gw[3:-3, 3:-3, -4].any()     # w tendencies on the two walls stay zero
    model.set_option("tendency_impl", 2)


def test_projection_and_conservation_at_config2(ocn, big_ppb):
    """test/test_time_stepping.jl:124-160,432-460 (max|div u| < 5e-8 on a stretched grid) and :165-199 (tracer conservation) at the
    configuration's full size; w stays exactly zero on the walls"""
    grid, model = big_ppb
    dt = 0.1 / N / 0.6
    from helpers import tanh_faces
    dz = np.diff(tanh_faces(N // 2))
    interior = (slice(3, -3),) * 3

    def volume_mean(a):
        return float((a[interior] * dz[None, None, :]).sum() / (dz.sum() * N * N))
    mean0 = {n: volume_mean(model.fields()[n].parent()) for n in ("T", "S")}
    for _ in range(3):
        ocn.time_step(model, dt)
    assert ocn.max_abs_divergence(model) < 5e-8
    for n in ("T", "S"):
        assert abs(volume_mean(model.fields()[n].parent()) - mean0[n]) < 1e-13 * max(1.0, abs(mean0[n])), n
    w = model.fields()["w"].parent()
    assert not w[3:-3, 3:-3, 3].any() and not w[3:-3, 3:-3, 3 + N // 2].any()


def test_fused_substep_equals_separate_kernels_at_config2(ocn, big_ppb):
    grid, model = big_ppb
    dt = 0.1 / N / 0.6
    start = {n: f.parent() for n, f in model.fields().items()}
    results = []
    for fuse in (1, 0):
        for n, f in model.fields().items():
            f.set_parent(start[n])
        ocn.update_state(model, True)
        model.set_option("fuse_substep", fuse)
        for _ in range(2):
            ocn.time_step(model, dt)
        results.append({n: f.parent().copy() for n, f in model.fields().items()})
    model.set_option("fuse_substep", 1)
    for n in results[0]:
        assert np.array_equal(results[0][n], results[1][n]), n


def test_config4_physics_at_config2_size(ocn, arch):
    """the physics of BASELINE.json configs[4] (AnisotropicMinimumDissipation, linear SeawaterBuoyancy with the hydrostatic pressure
    anomaly, wind-stress / heat-flux / bottom-gradient conditions, the S-dependent evaporation flux) at 256 x 256 x 128 stretched:
    size-independent properties -- the one-pass epilogue + fused substep leave the same bits as the stand-alone kernels + rk3_substep!,
    max|div u| < 5e-8 (test_time_stepping.jl:124-160), the eddy diffusivities are non-negative and finite and not all zero
    (anisotropic_minimum_dissipation.jl:199-357: max(0, .)), and the heat budget closes to the surface flux up to the diffusive flux the
    bottom Gradient condition lets through (kappa_e dT/dz there: bounded by max kappa_e * 0.01)"""
    from helpers import tanh_faces
    sys_path_bench = __import__("importlib").import_module("bench")
    size = (N, N, N // 2)
    z = tanh_faces(size[2])
    outs, budget = [], None
    for fused in (1, 0):
        grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), **sys_path_bench.workload_physics(ocn, "ppb_amd"))
        model.set_option("fused_epilogue", fused)
        model.set_option("fuse_substep", fused)
        ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=1234))
        dz = np.diff(z)[None, None, :]
        T0 = (model.fields()["T"].interior() * dz).sum()
        dt = 0.05 * grid.Δxᶜᵃᵃ / 0.6
        for _ in range(2):
            ocn.time_step(model, dt)
        assert ocn.max_abs_divergence(model) < 5e-8
        if fused:
            T1 = (model.fields()["T"].interior() * dz).sum()
            D = model.diffusivity_fields
            nu, kT = D[0].interior(), D[1][0].interior()
            assert np.isfinite(nu).all() and np.isfinite(kT).all() and nu.min() >= 0 and kT.min() >= 0 and nu.max() > 0 and kT.max() > 0
            budget = ((T1 - T0) / (size[0] * size[1]), -5e-5 * model.clock.time, float(kT.max()) * 0.01 * model.clock.time)
        outs.append({n: f.parent() for n, f in model.fields().items()} | {"p": model.pressures.pNHS.parent()})
        model.close()
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), n
    assert abs(budget[0] - budget[1]) <= budget[2] + 1e-12, budget


def _config2_pair_against_the_oracle(ocn, oracle, arch, label, physics=None, oracle_physics=None):
    """256 x 256 x 128, tanh_faces(128), (Periodic, Periodic, Bounded), helpers.smooth_state(seed = 1234): the product model and its
    oracle twin after ONE RK3 step at Δt = 0.1 Δx / 0.6, field by field (rel_err over the interior). u, v, w, T, S: north_star's 1e-12.
    p: two round-off-equivalent solvers differ by round-off times the condition number of the discrete Laplacian -- the error model of
    _slab_pair: max(1e-12, 4 eps cond), cond = λmax / λmin = (4/Δx² + 4/Δy² + 4/Δz_min²) / (2π/L)² -- the oracle itself moves p by 3.8e-12
    here under one last-bit perturbation of the initial velocities (u 6.0e-14, v 2.9e-14, w 1.9e-13, T 2.2e-16, S 2.5e-13)."""
    from helpers import field_pairs, rel_err, set_both, tanh_faces
    size = (N, N, N // 2)
    z = tanh_faces(size[2])
    g_gpu = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    g_cpu = oracle.Grid(size, topology=(oracle.PERIODIC, oracle.PERIODIC, oracle.BOUNDED), x=(0.0, 1.0), y=(0.0, 1.0), z=z)
    m_gpu = ocn.NonhydrostaticModel(grid=g_gpu, advection=ocn.WENO(), tracers=("T", "S"), **(physics or {}))
    m_cpu = oracle.Model(g_cpu, 2)
    if oracle_physics is not None:
        oracle_physics(m_cpu)
        # identical inputs (no projection round-off): the eddy viscosity and diffusivities, halos included, bit for bit -- as
        # test_anisotropic_minimum_dissipation_matches_oracle asserts at 16 x 16 x 12
        set_both(ocn, m_gpu, m_cpu, seed=1234, smooth=True, enforce_incompressibility=False)
        ocn.update_state(m_gpu, True)
        m_cpu.update_state(True)
        D = m_gpu.diffusivity_fields
        assert np.array_equal(D.νₑ.parent(), m_cpu.field("nu_e")) and m_cpu.field("nu_e").max() > 0
        for t, name in enumerate(("T", "S")):
            assert np.array_equal(getattr(D.κₑ, name).parent(), m_cpu.field("kappa_e%d" % t)) and m_cpu.field("kappa_e%d" % t).max() > 0, name
    set_both(ocn, m_gpu, m_cpu, seed=1234, smooth=True)
    dt = 0.1 * g_gpu.Δxᶜᵃᵃ / 0.6
    ocn.time_step(m_gpu, dt)
    m_cpu.time_step(dt)
    assert m_gpu.clock.time == m_cpu.time and ocn.max_abs_divergence(m_gpu) < 5e-8
    errs = {name: float(rel_err(a[3:-3, 3:-3, 3:-3], b[3:-3, 3:-3, 3:-3])) for name, a, b in field_pairs(m_gpu, m_cpu)}
    m_gpu.close()
    cond = (4.0 * size[0] ** 2 + 4.0 * size[1] ** 2 + 4.0 / float(np.diff(z).min()) ** 2) / (2 * np.pi) ** 2
    p_bound = max(1e-12, 4 * np.finfo(float).eps * cond)
    print(f"[{label}, 256x256x128 stretched, HIP vs oracle, 1 step] " + " ".join(f"{n}:{e:.2e}" for n, e in errs.items()) + f"  bound(p) = {p_bound:.2e}")
    for n in ("u", "v", "w", "T", "S"):
        assert errs[n] < 1e-12, errs
    assert errs["pNHS"] <= p_bound, (errs, cond)


def test_config2_against_the_oracle(ocn, oracle, arch):
    """BASELINE.json configs[2] at FULL size, HIP against the ORACLE field by field: the stretched metric tables, the Fourier-tridiagonal
    solve at Nz = 128 and the z-marching kernels over 256-wide planes are where an indexing error that depends on the size would live;
    the other full-size tests of this configuration compare kernel variants of the product with each other"""
    _config2_pair_against_the_oracle(ocn, oracle, arch, "configs[2]")


def test_config4_physics_against_the_oracle_at_config2_size(ocn, oracle, arch):
    """the physics of BASELINE.json configs[4] (bench.workload_physics(ocn, "ppb_amd"): AnisotropicMinimumDissipation, linear seawater
    buoyancy, wind stress / heat flux / bottom gradient / evaporation conditions) on the configs[2] grid, HIP against the ORACLE: νₑ, κₑ bit
    for bit on identical inputs (marching AMD kernel over 256-wide planes), then every field and the pressure after one RK3 step (marching
    epilogue, field-dependent flux condition, hydrostatic pressure anomaly)"""
    import bench

    def oracle_twin(m):         # bench.workload_physics(ocn, "ppb_amd"), one oracle call per entry
        m.set_amd()
        m.set_seawater_buoyancy(alpha=2e-4, beta=8e-4)
        m.set_bc("u", "top", "flux", -1e-4)
        m.set_bc("c0", "top", "flux", 5e-5)
        m.set_bc("c0", "bottom", "gradient", 0.01)
        m.set_linear_flux_bc("c1", "top", 0.0, -1e-3 / 3600.0, "c1")
    _config2_pair_against_the_oracle(ocn, oracle, arch, "configs[4] physics", bench.workload_physics(ocn, "ppb_amd"), oracle_twin)


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE.json configs[3] / configs[4]: the LOCAL shape of one of 8 x-slabs, run through the partitioned code path by a one-rank
# RCCL communicator that is its own neighbour (ocn_dist_set_self_loop) -- against the single-GPU model on the same periodic slab
# ---------------------------------------------------------------------------------------------------------------------
def _slab_pair(ocn, arch, size, zfaces, physics):
    """x spans (0, 1) on the slab, so that the analytic state is periodic over it (cells are anisotropic; a state that jumps at the
    slab's ends would make the comparison a test of the WENO weights' conditioning, not of the code path). For the same reason S is
    used WITHOUT its offset of 35: the reference's smoothness indicators (weno_interpolants.jl:204-216) are sums of products of the
    values themselves, not of differences, so for S = 35 + O(1) on a 512-point direction beta ~ 1e-4 is the difference of terms
    ~ 1e3 and the weights amplify a 1e-14 perturbation of the advecting velocity (two correct pressure solvers differ by that) to
    5e-11 in S after one step and 7e-10 after three (measured, tools/diag_slab.py: 64 x 512 x 512; 7e-13 / 1e-11 at 64 x 128 x 128;
    2e-15 with the offset removed). A property of the reference's formulation, the same in the oracle."""
    import ctypes as C
    from oldoceananigans_jl_amd import _lib, distributed as dist
    topo = (ocn.Periodic, ocn.Periodic, ocn.Periodic if zfaces is None else ocn.Bounded)
    z = (0.0, 1.0) if zfaces is None else zfaces
    uid = C.create_string_buffer(128)
    _lib.check(_lib.lib().ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    outs = []
    dt = 0.1 * (1.0 / size[1]) / 0.6
    for partitioned in (True, False):
        if partitioned:
            grid = dist.DistributedRectilinearGrid(ctx, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=topo)
            model = dist.LibraryDistributedModel(grid=grid, tracers=("T", "S"), **physics(ocn))
            nodes = {n: grid.global_nodes(f.loc) for n, f in model.fields().items()}
        else:
            grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=topo)
            model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), **physics(ocn))
            nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
        vals = smooth_state(nodes, seed=99)
        vals["S"] = vals["S"] - 35.0          # see the docstring: conditioning of the WENO weights of a tracer with a large offset
        ocn.set_model(model, **vals)
        for _ in range(2):
            ocn.time_step(model, dt)
        assert ocn.max_abs_divergence(model) < 5e-8
        out = {n: f.parent() for n, f in model.fields().items()}
        out["p"] = model.pressures.pNHS.parent()
        outs.append(out)
        model.close()
    ctx.close()
    # error model of the pressure: two exact-arithmetic-equivalent solvers (substructured / transposed x solve vs the single-GPU FFT
    # or Fourier-tridiagonal solve) return solutions that differ by round-off times the condition number of the discrete Laplacian,
    # lambda_max / lambda_min = (4/dx^2 + 4/dy^2 + 4/dz_min^2) / (2 pi / L)^2 -- 5e4 on the anisotropic 64 x 512 x 512 slab. The
    # velocities, which only see grad p, and the tracers keep the 1e-12 bar.
    dzmin = 1.0 / size[2] if zfaces is None else float(np.diff(np.asarray(zfaces)).min())
    cond = (4.0 * size[0] ** 2 + 4.0 * size[1] ** 2 + 4.0 / dzmin ** 2) / (2 * np.pi) ** 2
    for n in outs[0]:
        a, b = outs[0][n][3:-3, 3:-3, 3:-3], outs[1][n][3:-3, 3:-3, 3:-3]
        err = np.abs(a - b).max() / np.abs(b).max()
        assert err <= (1e-12 if n != "p" else max(1e-12, 4 * np.finfo(float).eps * cond)), (n, err, cond)
        if n != "p":
            assert np.array_equal(outs[0][n][:3, 3:-3, 3:-3], outs[0][n][-6:-3, 3:-3, 3:-3]), n     # exchanged x halos: exact copies


def test_config3_local_slab_through_the_partitioned_path(ocn, arch):
    """512^3 over Partition(8): the local 64 x 512 x 512 slab (thin slab: no interior / buffer split, substructured x solve)"""
    _slab_pair(ocn, arch, (64, 512, 512), None, lambda ocn: {})


def test_config4_local_slab_through_the_partitioned_path(ocn, arch):
    """1024 x 1024 x 256 over Partition(8) with the ocean_wind_mixing_and_convection physics: the local 128 x 1024 x 256 slab
    (stretched Bounded z, transposing Fourier-tridiagonal solver, AMD closure evaluated in the x-halo columns, linear seawater
    buoyancy, wind-stress / heat-flux / bottom-gradient / evaporation conditions)"""
    from helpers import tanh_faces

    def physics(ocn):
        F = ocn.FieldBoundaryConditions
        return dict(closure=ocn.AnisotropicMinimumDissipation(),
                    buoyancy=ocn.SeawaterBuoyancy(ocn.LinearEquationOfState(thermal_expansion=2e-4, haline_contraction=8e-4)),
                    coriolis=ocn.FPlane(f=1e-4),
                    boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-4)),
                                         "T": F(top=ocn.FluxBoundaryCondition(5e-5), bottom=ocn.GradientBoundaryCondition(0.01)),
                                         "S": F(top=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(b=-1e-3 / 3600.0), field_dependencies="S"))})
    _slab_pair(ocn, arch, (128, 1024, 256), tanh_faces(256), physics)


def test_config3_global_512_cubed_over_8_ranks(ocn, arch, monkeypatch):
    """BASELINE.json configs[3] at FULL size as a GLOBAL problem: 512^3 triply periodic over Partition(8) -- eight ranks of the library's
    partitioned model (64 x 512 x 512 each: halo pack / exchange / unpack, early exchange, substructured x solve with its all-gather),
    run as threads that share the one card over the caller-supplied transport (tests/loopback.py; RCCL itself needs eight cards) --
    against the single-GPU model on the 512^3 grid: every rank's slab of every field after two RK3 steps."""
    import test_gpu_dist_library as T
    from dist_worker import analytic as base_analytic
    # S without its offset of 35: see _slab_pair (conditioning of the reference's smoothness indicators on a 512-point direction)
    monkeypatch.setattr(T, "analytic", lambda name, x, y, z: base_analytic(name, x, y, z) - (35.0 if name == "S" else 0.0))
    T._own_stream()
    size, R, nsteps = (512, 512, 512), 8, 2
    results = T._run_library_ranks(ocn, arch, R, size, nsteps, "periodic", {})
    host = [(out, div, t) for out, div, t, _ in results]
    del results
    ref, time, _ = T._single_gpu(ocn, arch, size, "periodic", nsteps)
    nxl = size[0] // R
    dmin = min(2.0 / size[0], 1.0 / size[1], 1.0 / size[2])
    cond = (3 * 4.0 / dmin ** 2) / (2 * np.pi / 2.0) ** 2          # lambda_max / lambda_min of the discrete Laplacian (error model of p)
    for r, (out, div, t) in enumerate(host):
        assert div < 5e-8 and t == time
        for name, a in out.items():
            want = ref[name][3 + r * nxl:3 + (r + 1) * nxl, 3:-3, 3:-3]
            err = np.abs(a[3:-3, 3:-3, 3:-3] - want).max() / np.abs(ref[name]).max()
            assert err <= (1e-12 if name != "p" else max(1e-12, 4 * np.finfo(float).eps * cond)), (r, name, err)
        # exchanged x halos are exact copies of the neighbour's interior columns
        for name in ("u", "T"):
            east = host[(r + 1) % R][0][name]
            assert np.array_equal(out[name][-3:, 3:-3, 3:-3], east[3:6, 3:-3, 3:-3]), (r, name)


def test_config4_global_1024x1024x256_over_8_ranks(ocn, arch, monkeypatch):
    """BASELINE.json configs[4] at FULL size as a GLOBAL problem: 1024 x 1024 x 256, stretched Bounded z, the
    ocean_wind_mixing_and_convection physics (AnisotropicMinimumDissipation evaluated in the x-halo columns, linear seawater buoyancy,
    wind stress / heat flux / bottom gradient / evaporation conditions), eight ranks of 128 x 1024 x 256 through the library's
    partitioned step (transposing Fourier-tridiagonal solver: two all-to-alls per solve) as threads sharing the card, against the
    single-GPU model on the global grid after two RK3 steps."""
    import test_gpu_dist_library as T
    from dist_worker import analytic as base_analytic
    monkeypatch.setattr(T, "analytic", lambda name, x, y, z: base_analytic(name, x, y, z) - (35.0 if name == "S" else 0.0))
    T._own_stream()
    size, R, nsteps = (1024, 1024, 256), 8, 2
    results = T._run_library_ranks(ocn, arch, R, size, nsteps, "amd", {})
    host = [(out, div, t) for out, div, t, _ in results]
    del results
    ref, time, _ = T._single_gpu(ocn, arch, size, "amd", nsteps)
    nxl = size[0] // R
    from helpers import tanh_faces
    dzmin = float(np.diff(tanh_faces(size[2])).min())
    cond = (4.0 / (2.0 / size[0]) ** 2 + 4.0 * size[1] ** 2 + 4.0 / dzmin ** 2) / (2 * np.pi / 2.0) ** 2
    for r, (out, div, t) in enumerate(host):
        assert div < 5e-8 and t == time
        for name, a in out.items():
            want = ref[name][3 + r * nxl:3 + (r + 1) * nxl, 3:-3, 3:-3]
            err = np.abs(a[3:-3, 3:-3, 3:-3] - want).max() / np.abs(ref[name]).max()
            assert err <= (1e-12 if name != "p" else max(1e-12, 4 * np.finfo(float).eps * cond)), (r, name, err)


# ---------------------------------------------------------------------------------------------------------------------
# The survey's OWN inputs, S = 35 + sin(2 pi x) cos(2 pi y) UNCHANGED (tests/offset_tracer.py): the bound that holds instead of 1e-12
# ---------------------------------------------------------------------------------------------------------------------
def test_config1_survey_state_against_the_oracle_at_256(ocn, oracle, arch):
    """BASELINE.json configs[1] at full size, SURVEY.md 8(d)'s state exactly as written, HIP against the ORACLE field by field after one
    RK3 step (the oracle takes ~2.5 s per step here): u, v, w, T within north_star's 1e-12; S -- whose reference smoothness indicators are
    pure round-off on the lines where it is exactly uniform -- within the bound MEASURED on the oracle at this size: 4 x its largest movement
    under a last-bit perturbation of the initial velocities (seeds 7, 8; the unperturbed run is the one compared with), itself below the
    formula `offset_tracer_bound` (tests/offset_tracer.py::check_offset_tracer). The measured values are printed for DESIGN.md 3."""
    from helpers import make_pair, field_pairs, rel_err
    from offset_tracer import ORACLE_NAMES, check_offset_tracer, measured_offset_tracer_bound, offset_tracer_bound, survey_state
    size = (N, N, N)
    g_gpu, g_cpu, m_gpu, m_cpu = make_pair(ocn, oracle, arch, size)
    vals = survey_state({n: g_gpu.nodes(f.loc) for n, f in m_gpu.fields().items()})
    ocn.set_model(m_gpu, **vals)
    m_cpu.set(**{cn: vals[gn] for cn, gn in zip(["u", "v", "w", "c0", "c1"], m_gpu.fields().keys())})
    dt = 0.1 / N / 0.6
    ocn.time_step(m_gpu, dt)
    m_cpu.time_step(dt)
    errs = {name: rel_err(a[3:-3, 3:-3, 3:-3], b[3:-3, 3:-3, 3:-3]) for name, a, b in field_pairs(m_gpu, m_cpu)}
    assert ocn.max_abs_divergence(m_gpu) < 5e-8
    S_gpu = m_gpu.fields()["S"].interior()
    m_gpu.close()
    baseline = [{k: g_cpu.interior_cells(m_cpu.field(cn)).copy() for k, cn in ORACLE_NAMES.items()}]
    measured, raw = measured_offset_tracer_bound(oracle, size, 1, {k: np.asarray(vals[k]) for k in ORACLE_NAMES}, seeds=(7, 8), margin=4.0,
                                                 baseline=baseline)
    print("[survey state, 256^3, HIP vs oracle, 1 step] " + " ".join(f"{n}:{e:.2e}" for n, e in errs.items()) +
          f"  oracle sensitivity of S (seeds 7, 8) = {raw[0]:.2e}, {raw[1]:.2e}  ratio = {errs['S'] / max(raw):.2f}"
          f"  measured bound(S) = {measured:.2e}  formula = {offset_tracer_bound(size, 1):.2e}")
    for n in ("u", "v", "w", "T"):
        assert errs[n] < 1e-12, errs
    check_offset_tracer(S_gpu, baseline[0]["S"], measured, size, 1)


def test_config3_local_slab_with_the_survey_state_unchanged(ocn, oracle, arch):
    """configs[3]'s local 64 x 512 x 512 slab through the partitioned path (self-loop over RCCL, substructured x solve) against the
    single-GPU model, with S = 35 + sin cos UNCHANGED: two correct pressure solvers that differ at round-off. u, v, w, T within 1e-12
    (pressure within its condition-number bound); S within the bound MEASURED on the oracle on this very slab (4 x its largest movement
    after the same two steps under a last-bit perturbation of the initial velocities, seeds 7 and 8), itself below the formula
    `offset_tracer_bound` -- 1e-12 does not hold for it on a 512-point direction, in any implementation (weno_interpolants.jl:204-216).
    test_config3_local_slab_through_the_partitioned_path keeps the S - 35 variant."""
    import ctypes as C
    from oldoceananigans_jl_amd import _lib, distributed as dist
    from offset_tracer import check_offset_tracer, measured_offset_tracer_bound, offset_tracer_bound, survey_state
    size, nsteps = (64, 512, 512), 2
    uid = C.create_string_buffer(128)
    _lib.check(_lib.lib().ocn_dist_unique_id(uid))
    ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
    outs = []
    dt = 0.1 * (1.0 / size[1]) / 0.6
    for partitioned in (True, False):
        if partitioned:
            grid = dist.DistributedRectilinearGrid(ctx, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
            model = dist.LibraryDistributedModel(grid=grid, tracers=("T", "S"))
            nodes = {n: grid.global_nodes(f.loc) for n, f in model.fields().items()}
        else:
            grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0))
            model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"))
            nodes = {n: grid.nodes(f.loc) for n, f in model.fields().items()}
        state = survey_state(nodes, seed=99)
        ocn.set_model(model, **state)
        for _ in range(nsteps):
            ocn.time_step(model, dt)
        assert ocn.max_abs_divergence(model) < 5e-8
        outs.append({n: f.interior() for n, f in model.fields().items()})
        model.close()
    ctx.close()
    errs = {n: float(np.abs(outs[0][n] - outs[1][n]).max() / np.abs(outs[1][n]).max()) for n in outs[0]}
    measured, raw = measured_offset_tracer_bound(oracle, size, nsteps, {k: np.asarray(a) for k, a in state.items()}, seeds=(7, 8), margin=4.0)
    print(f"[survey state, 64x512x512 slab, partitioned vs single GPU, {nsteps} steps] " + " ".join(f"{n}:{e:.2e}" for n, e in errs.items()) +
          f"  oracle sensitivity of S (seeds 7, 8) = {raw[0]:.2e}, {raw[1]:.2e}  ratio = {errs['S'] / max(raw):.2f}"
          f"  measured bound(S) = {measured:.2e}  formula = {offset_tracer_bound(size, nsteps):.2e}")
    for n in ("u", "v", "w", "T"):
        assert errs[n] < 1e-12, errs
    check_offset_tracer(outs[0]["S"], outs[1]["S"], measured, size, nsteps)


def test_marching_amd_kernel_equals_the_per_cell_kernel_at_config2_size(ocn, arch):
    """AnisotropicMinimumDissipation's eddy coefficients at 256 x 256 x 128 (stretched Bounded z): the z-marching kernel that evaluates
    every point operand once (x neighbours by lane moves, z neighbours carried in registers, per-level factors from an LDS table;
    amd_diffusivities_march_kernel) against the one-thread-per-cell kernel that recomputes everything (option amd_march = 0; bit-identical
    to the oracle at small sizes, tests/test_gpu_parity.py) -- every cell of ν_e, κ_e(T), κ_e(S) bit for bit, also on a range that reaches
    into the x halos like the one an x-slab rank evaluates"""
    from helpers import tanh_faces
    grid = ocn.RectilinearGrid(arch, size=(N, N, N // 2), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N // 2),
                               topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    closure = ocn.AnisotropicMinimumDissipation()
    model = ocn.NonhydrostaticModel(grid=grid, tracers=("T", "S"), closure=closure)
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=3))
    flds = list(model.fields().values())
    outs = []
    for rng in (None, (0, N + 1, 1, N, 1, N // 2)):
        for march in (1, 0):
            ocn.set_option("amd_march", march)
            try:
                nu, ka = ocn.CenterField(grid), [ocn.CenterField(grid), ocn.CenterField(grid)]
                ocn.kernels.compute_amd_diffusivities(grid, closure, ("T", "S"), flds, nu, ka, kernel_parameters=rng)
                outs.append([nu.parent()] + [k.parent() for k in ka])
            finally:
                ocn.set_option("amd_march", 1)
        for a, b in zip(outs[-2], outs[-1]):
            assert np.array_equal(a, b) and np.isfinite(a).all() and a.max() > 0
    model.close()


@pytest.mark.parametrize("case", ["configs4_physics_256x256x128", "walls_scalar_diffusivity", "walls_no_tracer_amd"])
def test_marching_epilogue_equals_the_one_thread_per_value_epilogue(ocn, arch, case):
    """the pass that completes the tendencies after the advective part -- Coriolis, pHY′ gradient, closure fluxes, Flux conditions, the next
    stage's substep -- as a z-march that evaluates the symmetric viscous flux tensor once per point (tendency_epilogue_march_kernel + the
    boundary-cell kernel for Flux conditions, csrc/ocn_epilogue_march.h) against the one-thread-per-field-value kernel (option epilogue_march
    = 0; both bit-identical to the oracle at small sizes, tests/test_gpu_parity.py): fields, tendencies and pressure after 2 RK3 steps, bit for
    bit -- at the bench's configs[4]-physics size, and on wall-bounded grids with Flux conditions on every kind of side, sizes that are no
    multiple of the 62 columns / 4 rows a block covers"""
    from helpers import tanh_faces
    F = ocn.FieldBoundaryConditions
    if case == "configs4_physics_256x256x128":
        import bench
        grid = ocn.RectilinearGrid(arch, size=(N, N, N // 2), x=(0.0, 1.0), y=(0.0, 1.0), z=tanh_faces(N // 2), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
        kw = dict(tracers=("T", "S"), coriolis=ocn.FPlane(f=1e-4), **bench.workload_physics(ocn, "ppb_amd"))
        dt = 0.1 / N / 0.6
    elif case == "walls_scalar_diffusivity":
        grid = ocn.RectilinearGrid(arch, size=(70, 37, 21), x=(0.0, 1.0), y=(0.0, 0.6), z=tanh_faces(21), topology=(ocn.Bounded, ocn.Bounded, ocn.Bounded))
        kw = dict(tracers=("T", "S"), closure=ocn.ScalarDiffusivity(ν=2e-3, κ=1e-3), coriolis=ocn.FPlane(f=0.4), buoyancy=ocn.SeawaterBuoyancy(),
                  boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-3), south=ocn.FluxBoundaryCondition(2e-3)),
                                       "v": F(east=ocn.FluxBoundaryCondition(3e-3), bottom=ocn.FluxBoundaryCondition(-2e-3)),
                                       "w": F(west=ocn.FluxBoundaryCondition(1e-3), north=ocn.FluxBoundaryCondition(-1e-3)),
                                       "T": F(top=ocn.FluxBoundaryCondition(4e-3), west=ocn.FluxBoundaryCondition(-3e-3), north=ocn.FluxBoundaryCondition(2e-3)),
                                       "S": F(top=ocn.FluxBoundaryCondition(ocn.LinearFieldFlux(b=-2.5e-3), field_dependencies="S"), east=ocn.FluxBoundaryCondition(1e-3))})
        dt = 2e-3
    else:
        grid = ocn.RectilinearGrid(arch, size=(63, 9, 40), x=(0.0, 1.0), y=(0.0, 0.2), z=(0.0, 0.5), topology=(ocn.Periodic, ocn.Bounded, ocn.Bounded))
        kw = dict(tracers=(), closure=ocn.AnisotropicMinimumDissipation(), coriolis=ocn.FPlane(f=0.4),
                  boundary_conditions={"u": F(top=ocn.FluxBoundaryCondition(-1e-3)), "v": F(bottom=ocn.FluxBoundaryCondition(2e-3))})
        dt = 2e-3
    outs = []
    for march in (1, 0):
        ocn.set_option("epilogue_march", march)
        try:
            model = ocn.NonhydrostaticModel(grid=grid, **kw)
            ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=5))
            for _ in range(2):
                ocn.time_step(model, dt)
            out = {n: f.parent() for n, f in model.fields().items()}
            out.update({"G" + n: model.tendency(n).parent() for n in model.fields()})
            out["pNHS"] = model.pressures.pNHS.parent()
            outs.append(out)
            model.close()
        finally:
            ocn.set_option("epilogue_march", 1)
    for n in outs[0]:
        assert np.isfinite(outs[0][n]).all() and np.array_equal(outs[0][n], outs[1][n]), (case, n)
    assert np.abs(outs[0]["Gu"]).max() > 0


@pytest.mark.parametrize("size", [(1024, 1024, 256), (1024, 1024, 512)])
def test_role_kernel_on_parent_arrays_beyond_2_and_4_gib(ocn, arch, size):
    """288 GB of HBM hold single-GPU grids whose fields exceed the 31-bit byte offsets of the role kernel's buffer descriptors (1024 x 1024 x 256:
    2.2 GB per field) and the 32-bit ones of the all-fields kernel (1024 x 1024 x 512: 4.4 GB). Since round 3 a workgroup's descriptors start at
    the lowest plane of its own chunk, so the limit is on the plane, not on the array: the role kernel (default) against the per-field kernels
    (the reference's launch structure, FView's 64-bit indexing), whole parent arrays bit for bit. Fields are separable products set through
    set_parent (no projection: this is about addressing)."""
    grid = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    assert model.get_option("tendency_impl") == 2
    two_pi = 2 * np.pi
    for n, (name, f) in enumerate(model.fields().items()):
        P = f.shape
        ax = [np.arange(P[d]) / size[d] for d in range(3)]
        a = (np.sin(two_pi * ax[0] + 0.3 * n)[:, None, None] * np.cos(two_pi * ax[1] + 0.2 * n)[None, :, None]) * (1.0 + 0.25 * np.cos(two_pi * ax[2] + n))[None, None, :]
        f.set_parent(a + (0.5 if name in ("T", "S") else 0.0))
        del a
    want = None
    for impl in (2, 0):
        model.set_option("tendency_impl", impl)
        ocn.update_state(model, True)
        got = [model.tendency(n).parent() for n in model.fields()]
        if want is None:
            want = got
            continue
        for a, b, n in zip(want, got, model.fields()):
            assert np.array_equal(a, b), (size, n)
            assert np.isfinite(a).all() and np.abs(a[3:-3, 3:-3, -6]).max() > 0 and np.abs(a[3:-3, 3:-3, 3]).max() > 0
    model.set_option("tendency_impl", 2)
    model.close()


def test_marching_kernels_on_seeded_random_small_configurations(ocn, arch):
    """thirty seeded random small models -- sizes from 4 to 70 that are no multiple of a block's 62 columns / 4 rows / 16 levels, every mix of
    Periodic / Bounded directions, 0 to 2 tracers, ScalarDiffusivity or AnisotropicMinimumDissipation, with / without Coriolis and buoyancy,
    Flux conditions on random walls -- stepped twice with the z-marching epilogue and eddy-diffusivity kernels and with the one-thread-per-value
    kernels (options epilogue_march / amd_march = 0): fields, tendencies and pressure bit for bit"""
    from helpers import tanh_faces
    rng = np.random.default_rng(20251005)
    F = ocn.FieldBoundaryConditions
    ran = 0
    for case in range(30):
        size = tuple(int(rng.integers(4, 71 if d == 0 else 24)) for d in range(3))
        topo = tuple(ocn.Bounded if rng.random() < 0.5 else ocn.Periodic for _ in range(3))
        z = tanh_faces(size[2]) if (topo[2] is ocn.Bounded and rng.random() < 0.5) else (0.0, 0.7)
        ntr = int(rng.integers(0, 3))
        tracers = ("T", "S")[:ntr]
        amd = rng.random() < 0.5
        kw = dict(tracers=tracers, closure=ocn.AnisotropicMinimumDissipation() if amd else ocn.ScalarDiffusivity(ν=2e-3, κ=1e-3))
        if rng.random() < 0.5:
            kw["coriolis"] = ocn.FPlane(f=0.4)
        if ntr == 2 and rng.random() < 0.6:
            kw["buoyancy"] = ocn.SeawaterBuoyancy()
        elif ntr >= 1 and rng.random() < 0.3:
            kw["tracers"] = ("b",) + tracers[1:]
            kw["buoyancy"] = ocn.BuoyancyTracer()
        bcs = {}
        sides = {0: ("west", "east"), 1: ("south", "north"), 2: ("bottom", "top")}
        normal = {"u": 0, "v": 1, "w": 2}
        for name in ("u", "v", "w") + tuple(kw["tracers"]):
            conds = {}
            for d in range(3):
                if topo[d] is ocn.Bounded and normal.get(name) != d:
                    for sd in sides[d]:
                        if rng.random() < 0.35:
                            conds[sd] = ocn.FluxBoundaryCondition(float(rng.normal()) * 1e-3)
            if conds:
                bcs[name] = F(**conds)
        if bcs:
            kw["boundary_conditions"] = bcs
        grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 0.8), z=z, topology=topo)
        outs = []
        for march in (1, 0):
            ocn.set_option("epilogue_march", march)
            ocn.set_option("amd_march", march)
            try:
                model = ocn.NonhydrostaticModel(grid=grid, **kw)
                ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=100 + case))
                for _ in range(2):
                    ocn.time_step(model, 1e-3)
                out = {n: f.parent() for n, f in model.fields().items()}
                out.update({"G" + n: model.tendency(n).parent() for n in model.fields()})
                out["pNHS"] = model.pressures.pNHS.parent()
                outs.append(out)
                model.close()
            finally:
                ocn.set_option("epilogue_march", 1)
                ocn.set_option("amd_march", 1)
        for n in outs[0]:
            assert np.array_equal(outs[0][n], outs[1][n], equal_nan=True), (case, size, [t.__name__ for t in topo], kw.keys(), n)
        assert np.isfinite(outs[0]["u"]).all(), (case, size)
        ran += 1
    assert ran == 30
