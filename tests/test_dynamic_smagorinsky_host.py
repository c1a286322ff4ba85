"""CPU tests of the dynamic Smagorinsky coefficient: analytic known answers of the numpy restatement (tests/dynamic_smagorinsky_reference.py)
that the GPU kernels are compared with bit for bit, the two halo facts of the reference, the clamping case used on the GPU, and the host
mirror (constructors, reprs, averaging forms, refusals, the schedule). No device."""
import numpy as np
import pytest

import oldoceananigans_jl_amd as ocn

import dynamic_smagorinsky_reference as R

F, Cn = ocn.Face, ocn.Center
LOCS = {"u": (F, Cn, Cn), "v": (Cn, F, Cn), "w": (Cn, Cn, F)}
N = 12
INNER = (slice(2, N - 2),) * 3          # cells at least two away from every boundary: the unfilled halo of Σ plays no part


def _grid(dx=0.25, dy=0.25, dz=0.25, topology=ocn.Bounded):
    return ocn.RectilinearGrid(None, size=(N, N, N), x=(0.0, N * dx), y=(0.0, N * dy), z=(-N * dz, 0.0), topology=(topology,) * 3, halo=(3, 3, 3))


def _parent(grid, name, fn):
    """fn(x, y, z) at every node of the field's parent array (halos included: no fill is involved)"""
    lx, ly, lz = LOCS[name]
    x = (grid.xᶠᵃᵃ if lx is F else grid.xᶜᵃᵃ)[:, None, None]
    y = (grid.yᵃᶠᵃ if ly is F else grid.yᵃᶜᵃ)[None, :, None]
    z = (grid.zᵃᵃᶠ if lz is F else grid.zᵃᵃᶜ)[None, None, :]
    return np.asfortranarray(np.broadcast_to(fn(x, y, z), grid.total_size(LOCS[name])).astype(np.float64))


def _zero(grid, name):
    return _parent(grid, name, lambda x, y, z: 0.0 * (x + y + z))


# round-off of the closed forms below. Lᵢᵢ = filter(ℑ(uᵢ²)) - ℑ(ūᵢ²) is a difference of two numbers of size a² X², X <= 1.25 L the largest
# coordinate in the parent array, that leaves a² Δ² / 6 = a² L² / 864: a few roundings of 2⁻⁵³ on the operands are a relative error of
# 864 * 1.25² * (a few) * 1.1e-16 < 1e-12 of the result; the products LM, MM carry three such factors. 1e-10 leaves a factor of 30.
RTOL = 1e-10


def test_shear_u_of_y():
    """u = a y: Σ₁₂ = a / 2 and nothing else, Σ² = 2 ℑxy(Σ₁₂²) = a² / 2, Σ = |a| / √2. The filter reproduces a linear function, so ū = u,
    Σ̄ᵢⱼ = Σᵢⱼ, Σ̄ = Σ and Mᵢⱼ = 2 Δf² (1 - 4) Σ Σᵢⱼ: M₁₂ = -3 Δf² a |a| / √2, every other Mᵢⱼ = 0, MM = 2 M₁₂² = 9 Δf⁴ a⁴.
    L₁₁ = filter(a² y²) - a² y² = a² Δy² / 6 is the only Lᵢⱼ that does not vanish (v = w = 0), and it meets M₁₁ = 0: LM = 0."""
    g = _grid()
    m = R.Metrics(g)
    for a in (0.7, -1.3):
        u, v, w = _parent(g, "u", lambda x, y, z: a * y + 0.0 * (x + z)), _zero(g, "v"), _zero(g, "w")
        L, M = R.tensors(m, u, v, w)
        LM, MM = R.contract(L, M)
        df2 = m.df2[g.Hz]
        assert np.all(LM[INNER] == 0.0)
        assert np.allclose(MM[INNER], 9 * df2 * df2 * a ** 4, rtol=RTOL, atol=0.0)
        assert np.allclose(M[3][INNER], -3 * df2 * a * abs(a) / np.sqrt(2.0), rtol=RTOL, atol=0.0)
        assert np.allclose(L[0][INNER], a * a * g.Δyᵃᶜᵃ ** 2 / 6, rtol=RTOL, atol=0.0)


def test_plane_strain_u_of_x_w_of_z():
    """u = a x, w = -a z on a grid with Δx ≠ Δz: Σ₁₁ = a, Σ₃₃ = -a, Σ² = 2 a², Σ = √2 |a|; ū = u, w̄ = w, Σ̄ = Σ.
    u₁u₁ = ℑx(u²) = a² (x² + Δx² / 4) at the cell centre x; its filter adds the second difference over 12: filter(u₁u₁) = u₁u₁ + a² Δx² / 6,
    and ū₁ū₁ = u₁u₁, so L₁₁ = a² Δx² / 6; likewise L₃₃ = a² Δz² / 6. u₁u₃ = -a² x z is bilinear: its filter is itself and L₁₃ = 0 to
    round-off; L₂₂ = L₁₂ = L₂₃ = 0 exactly (v = 0).
    M₁₁ = 2 Δf² (1 - 4) Σ Σ₁₁ = -6 √2 Δf² |a| a, M₃₃ = +6 √2 Δf² |a| a, every other Mᵢⱼ = 0 (M₁₃ to round-off).
    LM = L₁₁ M₁₁ + L₃₃ M₃₃ = √2 Δf² |a| a³ (Δz² - Δx²),  MM = M₁₁² + M₃₃² = 144 Δf⁴ a⁴."""
    dx, dz = 0.25, 0.125
    g = _grid(dx=dx, dz=dz)
    m = R.Metrics(g)
    for a in (0.7, -1.3):
        u, v, w = _parent(g, "u", lambda x, y, z: a * x + 0.0 * (y + z)), _zero(g, "v"), _parent(g, "w", lambda x, y, z: -a * z + 0.0 * (x + y))
        L, M = R.tensors(m, u, v, w)
        LM, MM = R.contract(L, M)
        df2 = m.df2[g.Hz]
        m11 = -6 * np.sqrt(2.0) * df2 * abs(a) * a
        assert np.allclose(L[0][INNER], a * a * dx * dx / 6, rtol=RTOL, atol=0.0)
        assert np.allclose(L[2][INNER], a * a * dz * dz / 6, rtol=RTOL, atol=0.0)
        assert np.all(L[1][INNER] == 0.0) and np.all(L[3][INNER] == 0.0) and np.all(L[5][INNER] == 0.0)
        scale = a * a * (N * dx) * (N * dz)                       # the size of u₁u₃ that cancels in L₁₃
        assert np.all(np.abs(L[4][INNER]) < 1e-13 * scale)
        assert np.allclose(M[0][INNER], m11, rtol=RTOL, atol=0.0) and np.allclose(M[2][INNER], -m11, rtol=RTOL, atol=0.0)
        assert np.all(np.abs(M[4][INNER]) < 1e-13 * abs(m11)) and np.all(M[1][INNER] == 0.0)
        assert np.allclose(MM[INNER], 144 * df2 * df2 * a ** 4, rtol=RTOL, atol=0.0)
        assert np.allclose(LM[INNER], np.sqrt(2.0) * df2 * abs(a) * a ** 3 * (dz * dz - dx * dx), rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("mask", [3, 7, 0])
def test_fluid_at_rest_has_zero_viscosity(mask):
    """u = v = w = 0: MM = 0 everywhere, the quotient of the coefficient is Inf or NaN and is discarded: νₑ is exactly 0, never NaN --
    after the initialising update and (Lagrangian) after an averaging update"""
    g = _grid(topology=ocn.Periodic)
    u, v, w = (np.zeros(g.total_size(LOCS[n]), order="F") for n in "uvw")
    d = R.DynamicDriver(g, mask)
    d.update(u, v, w, 0.0, 0, np.inf)
    if mask == 0:
        assert np.all(d.J_LM == 1e-32) and np.all(d.J_MM == 0.0)
        d.update(u, v, w, 0.1, 1, 0.1)
        assert d.initialisations == 1 and d.updates == 2
        assert np.isfinite(d.J_LM).all() and np.all(d.J_MM == 0.0)
    else:
        assert np.all(d.MM == 0.0) and np.all(d.J_MM == 0.0)
    nu = d.viscosity(u, v, w)
    assert np.all(nu == 0.0) and not np.isnan(nu).any()


def _periodic_state(g):
    tau = 2 * np.pi / (N * 0.25)
    u = _parent(g, "u", lambda x, y, z: 0.5 * np.sin(tau * x) * np.cos(tau * y) * np.cos(2 * tau * z))
    v = _parent(g, "v", lambda x, y, z: -0.5 * np.cos(tau * x) * np.sin(tau * y) * np.cos(tau * z) + 0.1 * np.sin(tau * x))
    w = _parent(g, "w", lambda x, y, z: 0.2 * np.cos(tau * x) * np.cos(2 * tau * y) * np.sin(tau * z))
    return u, v, w


def test_the_halo_of_sigma_is_not_filled_even_on_a_periodic_grid():
    """the reference launches _compute_Σ! over the interior and fills no halo: next to a Periodic boundary filter(Σ Σᵢⱼ) reads 0 for the
    neighbour across it. LM in the boundary cells therefore differs from the value with Σ's halo filled periodically; one cell further in
    nothing differs"""
    g = _grid(topology=ocn.Periodic)
    m = R.Metrics(g)
    u, v, w = _periodic_state(g)
    Sig = R.sigma(m, u, v, w)
    H = g.Hx
    assert np.all(Sig[:H] == 0.0) and np.all(Sig[:, :, -H:] == 0.0) and np.all(Sig[H:-H, H:-H, H:-H] > 0.0)
    wrapped = np.asfortranarray(np.pad(Sig[H:-H, H:-H, H:-H], H, mode="wrap"))
    LM, MM = R.lm_mm(m, u, v, w)
    LMw, MMw = R.lm_mm(m, u, v, w, Sig=wrapped)
    inner = (slice(1, N - 1),) * 3
    assert np.array_equal(LM[inner], LMw[inner]) and np.array_equal(MM[inner], MMw[inner])
    boundary = np.ones((N, N, N), dtype=bool)
    boundary[inner] = False
    differs = LM[boundary] != LMw[boundary]
    assert differs.mean() > 0.9
    assert np.max(np.abs(LM[boundary] - LMw[boundary])) > 1e-3 * np.max(np.abs(LMw))


def test_the_lagrangian_halos_keep_the_initial_mean():
    """parent(𝒥) .= mean writes the halos once; an averaging update writes the interior only and the copy to 𝒥⁻ copies the parent"""
    g = _grid(topology=ocn.Periodic)
    u, v, w = _periodic_state(g)
    d = R.DynamicDriver(g, 0)
    d.update(u, v, w, 0.0, 0, np.inf)
    mean_lm, mean_mm = d.J_LM[0, 0, 0], d.J_MM[0, 0, 0]
    assert np.all(d.J_LM == mean_lm) and np.all(d.J_MM == mean_mm) and mean_mm > 0
    for step in (1, 2):
        d.update(u, v, w, 0.05 * step, step, 0.05)
    H = g.Hx
    halo = np.ones(d.J_LM.shape, dtype=bool)
    halo[H:-H, H:-H, H:-H] = False
    assert np.all(d.J_LM[halo] == mean_lm) and np.all(d.J_MM[halo] == mean_mm)
    assert np.all(d.J_LM_prev[halo] == mean_lm)
    assert not np.all(d.J_MM[~halo] == mean_mm)
    assert d.initialisations == 1 and d.updates == 3


def test_ordered_average_is_an_average():
    """the library's summation order restated: against math.fsum within the bound of a sum of n terms, and exact for dyadic numbers"""
    import math
    g = ocn.RectilinearGrid(None, size=(70, 6, 20), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded),
                            halo=(3, 3, 3))
    rng = np.random.default_rng(3)
    a = np.asfortranarray(rng.uniform(-1, 1, g.total_size((Cn, Cn, Cn))))
    inner = a[3:-3, 3:-3, 3:-3]
    for mask in range(1, 8):
        got = R.ordered_average(g, a, mask)
        axes = tuple(d for d in range(3) if mask >> d & 1)
        n = int(np.prod([inner.shape[d] for d in axes]))
        assert got.shape == tuple(1 if mask >> d & 1 else s for d, s in enumerate(inner.shape))
        want = np.mean(inner, axis=axes, keepdims=True)
        assert np.max(np.abs(got - want)) <= n * 2.0 ** -53
        dyadic = np.asfortranarray(np.round(a * 64) / 64)
        assert np.array_equal(R.ordered_sum(dyadic[3:-3, 3:-3, 3:-3], mask), np.sum(dyadic[3:-3, 3:-3, 3:-3], axis=axes, keepdims=True))
    assert abs(R.ordered_mean(g, a) - math.fsum(inner.ravel()) / inner.size) <= 2.0 ** -53


CLAMP_MASK = 1          # averaging along x: Ny Nz coefficients per case


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_the_clamping_case_clamps_part_of_the_coefficients(oracle, name):
    """the minimum_numerator of the GPU clamping test, chosen from the restatement's 𝒥ᴸᴹ: at least 10 % of the entries on each side"""
    g = R.make_grid(ocn, None, name)
    vals, _ = R.case_values(g, "none")
    from smagorinsky_reference import oracle_parents
    Pn = oracle_parents(oracle, name, vals)
    d = R.DynamicDriver(g, CLAMP_MASK)
    d.coefficient_update(Pn["u"], Pn["v"], Pn["w"])
    jmin = R.clamping_minimum(d.J_LM)
    clamped = float(np.mean(d.J_LM < jmin))
    assert 0.1 <= clamped <= 0.9 and float(np.mean(d.J_LM > jmin)) >= 0.1, clamped


# ---------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_reprs_are_the_reference_s():
    dc = ocn.DynamicCoefficient(averaging=(1, 2))
    assert repr(dc) == ("DynamicCoefficient with\n├── averaging = (1, 2)\n├── schedule = IterationInterval(1, 0)\n"
                        "└── minimum_numerator = 1.0e-32")
    assert dc.summary() == "DynamicCoefficient(averaging = (1, 2), schedule = IterationInterval(1, 0))"
    assert repr(ocn.Smagorinsky(coefficient=dc)) == ("Smagorinsky closure with\n├── coefficient = DynamicCoefficient(averaging = (1, 2), "
                                                     "schedule = IterationInterval(1, 0))\n└── Pr = 1.0")
    dc4 = ocn.DynamicCoefficient(averaging=(1, 2), schedule=ocn.IterationInterval(4))
    assert repr(dc4).splitlines()[2] == "├── schedule = IterationInterval(4, 0)"
    assert repr(ocn.Smagorinsky(coefficient=dc4)).splitlines()[1] == ("├── coefficient = DynamicCoefficient(averaging = (1, 2), "
                                                                      "schedule = IterationInterval(4, 0))")
    assert ocn.DynamicCoefficient(averaging=ocn.LagrangianAveraging()).summary().startswith("DynamicCoefficient(averaging = LagrangianAveraging()")
    assert ocn.DynamicCoefficient(averaging=ocn.Colon).summary().startswith("DynamicCoefficient(averaging = Colon()")
    assert ocn.DynamicCoefficient(averaging=1, minimum_numerator=1e-20).minimum_numerator == 1e-20
    assert ocn.Smagorinsky(coefficient=dc).summary() == "Smagorinsky with coefficient = " + dc.summary() + ", Pr=1.0"


@pytest.mark.parametrize("averaging,mask,kept", [(1, 1, 1), ((1, 2), 3, (1, 2)), ((2, 3), 6, (2, 3)), (ocn.Colon, 7, ocn.Colon), (":", 7, ocn.Colon),
                                                  (ocn.LagrangianAveraging(), 0, ocn.LagrangianAveraging())])
def test_averaging_forms(averaging, mask, kept):
    dc = ocn.DynamicCoefficient(averaging=averaging)
    assert dc.averaging_mask == mask and dc.averaging == kept
    c = ocn.DynamicSmagorinsky(averaging=averaging, Pr=2.0, schedule=ocn.IterationInterval(5, 2), minimum_numerator=1e-30)
    assert isinstance(c, ocn.Smagorinsky) and c.dynamic and c.Pr == 2.0 and c.buffer == 2
    assert c.coefficient.averaging_mask == mask and c.coefficient.schedule.interval == 5 and c.coefficient.schedule.offset == 2
    assert c.coefficient.minimum_numerator == 1e-30
    default = ocn.DynamicSmagorinsky(averaging=averaging)
    assert default.Pr == 1.0 and default.coefficient.schedule.interval == 1 and default.coefficient.minimum_numerator == 1e-32


def test_refusals():
    assert ocn.DynamicCoefficient().averaging is None                                   # it can still be written down
    with pytest.raises(NotImplementedError, match="averaging"):
        ocn.Smagorinsky(coefficient=ocn.DynamicCoefficient())
    with pytest.raises(NotImplementedError):
        ocn.SmagorinskyLilly(C=ocn.DynamicCoefficient(averaging=(1, 2)))
    with pytest.raises(NotImplementedError, match="IterationInterval"):
        ocn.Smagorinsky(coefficient=ocn.DynamicCoefficient(averaging=1, schedule=ocn.TimeInterval(1.0)))
    with pytest.raises(NotImplementedError, match="VerticallyImplicit"):
        ocn.DynamicSmagorinsky(ocn.VerticallyImplicitTimeDiscretization(), averaging=1)
    for bad in (0, 4, (1, 1), (1, 5), ()):
        with pytest.raises((ValueError, TypeError)):
            ocn.DynamicCoefficient(averaging=bad)
    for bad in (1.5, "x", True):
        with pytest.raises(TypeError):
            ocn.DynamicCoefficient(averaging=bad)
    with pytest.raises(TypeError):
        ocn.DynamicSmagorinsky()
    with pytest.raises(ValueError):
        ocn.DynamicSmagorinsky(averaging=1, Pr=0.0)
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    with pytest.raises(NotImplementedError):                                              # closure tuples
        ocn.NonhydrostaticModel(grid=grid, closure=(ocn.DynamicSmagorinsky(averaging=1), ocn.ScalarDiffusivity(ν=1e-3)))

    class Partitioned:                       # what the model constructor recognises a partitioned grid by
        local = grid
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.NonhydrostaticModel(grid=Partitioned(), closure=ocn.DynamicSmagorinsky(averaging=(1, 2)))


@pytest.mark.parametrize("interval,offset", [(1, 0), (3, 0), (3, 1)])
def test_schedule_over_the_updates_of_rk3(interval, offset):
    """RK3 updates the state three times per step: after stages 1 and 2 the clock still shows the old iteration, after stage 3 the new one
    (and once before the first step, at iteration 0). IterationInterval(n, offset) fires where (iteration - offset) % n == 0"""
    seen = [0]                                           # the update_state! before the first step
    for it in range(6):
        seen += [it, it, it + 1]
    fired = [R.schedule_fires(i, interval, offset) for i in seen]
    if interval == 1:
        assert all(fired)
    elif offset == 0:
        #        it 0   step 1 (0 0 1)   step 2 (1 1 2)   step 3 (2 2 3)   step 4 (3 3 4)   step 5 (4 4 5)   step 6 (5 5 6)
        assert fired == [True, True, True, False, False, False, False, False, False, True, True, True, False, False, False, False, False, False, True]
    else:
        assert fired == [False, False, False, True, True, True, False, False, False, False, False, False, True, True, True, False, False, False, False]

    class M:
        class clock:
            iteration = 0
    schedule = ocn.IterationInterval(interval, offset)
    for i, f in zip(seen, fired):
        M.clock.iteration = i
        assert schedule(M) == f
    # the driver moves previous_compute_time on every call, fired or not
    g = _grid(topology=ocn.Periodic)
    u, v, w = (np.zeros(g.total_size(LOCS[n]), order="F") for n in "uvw")
    d = R.DynamicDriver(g, 3, interval=interval, offset=offset)
    for n, i in enumerate(seen[:7]):
        assert d.update(u, v, w, 0.1 * n, i, 0.1) == fired[n]
        assert d.previous_time == 0.1 * n


def test_a_restarted_lagrangian_average_initialises():
    """a restored model: the clock shows a time > 0 and a finite last_Δt, and the 𝒥 fields hold nothing. The first update that fires
    initialises -- also when it is not the first call (IterationInterval(5) restored at iteration 52 fires at 55) -- and later ones average;
    without it 𝒥⁻ = 0 gives T⁻ = Inf, ε = 0, 𝒥ᴹᴹ = 0 and νₑ = 0 for ever"""
    g = _grid(topology=ocn.Periodic)
    u, v, w = _periodic_state(g)
    d = R.DynamicDriver(g, 0)
    d.restart(5.0)
    assert d.update(u, v, w, 5.0, 50, 0.05) and d.initialisations == 1
    for n in (1, 2):
        assert d.update(u, v, w, 5.0 + 0.05 * n, 50 + n, 0.05)
    assert d.initialisations == 1 and d.updates == 3 and len(d.clamped) == 2
    assert d.J_MM.min() > 0 and d.viscosity(u, v, w).max() > 0
    d = R.DynamicDriver(g, 0, interval=5)
    d.restart(5.2)
    fired = [d.update(u, v, w, 5.2 + 0.05 * n, 52 + n, 0.05) for n in range(5)]
    assert fired == [False, False, False, True, False] and d.initialisations == 1 and d.updates == 1
    assert d.J_MM.min() > 0 and np.all(d.J_MM == d.J_MM[0, 0, 0])
