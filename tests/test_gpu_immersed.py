"""ImmersedBoundaryGrid on the MI355X against the numpy restatement (tests/immersed_reference.py, pinned to the oracle on the CPU by
tests/test_immersed_host.py), on the grids of tests/immersed_cases.py:

  1. the two flag tables of ocn_grid_get_immersed_flags == the restatement, every entry of the parent extent;
  2. Gu, Gv, Gw, Gc after update_state == the restatement, bitwise, from a projected smooth state, without and with
     ScalarDiffusivity(ν != κ); the raw entry points on random arrays;
  3. a model on ImmersedBoundaryGrid(grid, GridFittedBottom(below the domain)) == the plain model on the same grid, every field and pNHS,
     after 3 RK3 and 3 AB2 steps;
  4. 3 RK3 and 3 AB2 steps against ImmersedOrchestrated (BuoyancyTracer, FPlane, ScalarDiffusivity, an array forcing, a Flux condition on
     the top) to 1e-12, and where the masks leave exact zeros; a triply periodic grid; SeawaterBuoyancy with Value, Gradient and function
     Flux conditions; a forcing program, cell_advection_timescale, TimeStepWizard and Simulation;
  5. no flux through the solid: the drift of the tracer content of the active cells against the yardstick's;
  6. the reference's Gaussian immersed diffusion (test/test_dynamics.jl:89-116);
  7. the answers of the new entry points.

Path 2 (the flux-sharing role kernel) serves G1, G4 and G5 -- periodic in x and y, no Flat direction -- and is what their models take
by default; tendency_impl = 0 forces path 1 (one field per launch), the only path of G2 and G3.

G1 .. G5 are one partial tile of that kernel (64 x 7 cells, an eighth wave for the flux lines of row j0 + 7 and column i0 + 64). The
tile-edge cases T1 .. T6 of tests/immersed_cases.py put immersed cells on both sides of every tile seam and run, on path 2: the tables;
the raw entry on random arrays (beside path 1), over trimmed ranges and at every chunk length; the model's tendencies without and with
the closure; path 2 against path 1 over 2 steps; one step against the yardstick on T1."""
import ctypes as C
import warnings

import numpy as np
import pytest

import immersed_cases as IC
import immersed_reference as IR
import vertically_implicit_reference as R
from helpers import rel_err, smooth_state

pytestmark = pytest.mark.gpu

NU, KAPPA, FCOR = 2e-3, 5e-3, 0.7
PATH2 = ("G1", "G4", "G5")
_shared = {}


@pytest.fixture
def tendency_impl(ocn):
    """sets the library default of tendency_impl (what new models copy) and restores it"""
    def set_(v):
        ocn.set_option("tendency_impl", v)
    yield set_
    ocn.set_option("tendency_impl", 2)


def _restatement(ocn, case, boundary=None):
    """the restatement's predicates and tables for a case, computed once"""
    key = (case, "empty" if boundary is not None else "own")
    if key not in _shared:
        grid = IC.underlying_grid(ocn, None, case)
        m = R.Metrics.of_grid(grid)
        _shared[key] = IR.Immersed(m, IR.cells_of_grid(grid, IC.case_of(case)["boundary"] if boundary is None else boundary, m)[0])
    return _shared[key]


@pytest.fixture
def role_kchunk(ocn):
    """sets the library default of role_kchunk (what the raw entry points read) and restores it"""
    def set_(v):
        ocn.set_option("role_kchunk", v)
    yield set_
    ocn.set_option("role_kchunk", 0)


def _model(ocn, grid, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # the FFT-solver warning of an immersed model (tests/test_immersed_host.py)
        return ocn.NonhydrostaticModel(grid=grid, **kw)


def _state(grid, model, seed):
    vals = smooth_state({("T" if n == "b" else n): grid.nodes(f.loc) for n, f in model.fields().items()}, seed)
    if "T" in vals and "b" in model.fields():
        vals["b"] = vals.pop("T")
    return vals


def _core(m, a):
    """the interior of a parent array, immersed cells included"""
    return a[tuple(slice(h, s - h) for h, s in zip(m.H, a.shape))]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the flag tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(IC.CASES))
def test_flag_tables_are_the_restatement(ocn, arch, case):
    ibg = IC.immersed_grid(ocn, arch, case)
    imm = _restatement(ocn, case)
    periphery, orders = ibg.immersed_flags()
    assert periphery.shape == imm.periphery.shape and orders.dtype == np.uint16
    assert np.array_equal(periphery, imm.periphery), np.argwhere(periphery != imm.periphery)[:5]
    assert np.array_equal(orders, imm.orders), np.argwhere(orders != imm.orders)[:5]
    inside = _core(imm.m, periphery)
    assert (inside & 1).any() and ((inside >> 1) != 0).any()
    # every cascade level occurs along z (the boundary) on both sides
    for side in (0, 1):
        assert set(np.unique((_core(imm.m, orders) >> (2 * (4 + side))) & 3)) == {1, 2, 3}


@pytest.mark.parametrize("case", list(IC.TILE_CASES))
def test_tile_flag_tables_are_the_restatement(ocn, arch, case):
    """the two tables on the tile-edge cases, halo entries included: the edge wave of the flux-sharing kernel reads column Nx + 1 and row
    Ny + 1 (what the cases hold at the seams: tests/test_immersed_host.py::test_tile_cases_hold_what_they_promise)"""
    imm = _restatement(ocn, case)
    periphery, orders = IC.immersed_grid(ocn, arch, case).immersed_flags()
    assert np.array_equal(periphery, imm.periphery), np.argwhere(periphery != imm.periphery)[:5]
    assert np.array_equal(orders, imm.orders), np.argwhere(orders != imm.orders)[:5]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the tendencies
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = [(c, closure, path) for c in IC.CASES for closure in (False, True) for path in ((1, 2) if c in PATH2 else (1,))]


@pytest.mark.parametrize("case,closure,path", VARIANTS, ids=[f"{c}-{'with_closure' if cl else 'advection'}-path{p}" for c, cl, p in VARIANTS])
def test_tendencies_are_the_restatement(ocn, arch, tendency_impl, case, closure, path):
    """after set! (masked, projected) and update_state! the stage tendencies == the restatement evaluated on the model's own halo-filled
    fields, bit for bit over the whole parent array: the immersed cascade, the conditional fluxes, the conditional closure fluxes -- by the
    per-field kernels (path 1) and, where it applies, by the flux-sharing kernel (path 2)"""
    _tendencies_are_the_restatement(ocn, arch, tendency_impl, case, closure, path)


@pytest.mark.parametrize("closure", [False, True], ids=["advection", "with_closure"])
@pytest.mark.parametrize("case", list(IC.TILE_CASES))
def test_tile_tendencies_are_the_restatement(ocn, arch, tendency_impl, case, closure):
    """the same on the tile-edge cases by the flux-sharing kernel (path 2): several tiles, the edge wave's two flux lines and its flag
    reads live, immersed cells on both sides of every tile seam"""
    _tendencies_are_the_restatement(ocn, arch, tendency_impl, case, closure, 2)


def _tendencies_are_the_restatement(ocn, arch, tendency_impl, case, closure, path):
    tendency_impl(2 if path == 2 else 0)
    ibg = IC.immersed_grid(ocn, arch, case)
    imm = _restatement(ocn, case)
    m = imm.m
    model = _model(ocn, ibg, tracers=("b",), closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA) if closure else None)
    assert model.get_option("immersed") == 1 and model.get_option("immersed_tendency_path") == path
    for key in ("fuse_substep_active", "substep_in_tendency_kernel", "epilogue_march_active", "halo_fill_folded", "stage1_source_fused",
                "fused_tendency_active"):
        assert model.get_option(key) == 0, key
    ocn.set_model(model, **_state(ibg, model, 7))
    ocn.update_state(model)
    U = {cn: model.fields()[n].parent() for cn, n in zip(("u", "v", "w", "c"), ("u", "v", "w", "b"))}
    # the masks: the tracer is exactly zero at its immersed nodes; so were the velocities when set! masked them, before the projection
    cells = _core(m, imm.cell)
    assert np.all(_core(m, U["c"])[cells] == 0.0) and cells.any()
    adv = (U["u"], U["v"], U["w"])
    for cn, n in zip(("u", "v", "w", "c"), ("u", "v", "w", "b")):
        want = IR.advective_tendency(m, imm, cn, adv, U[cn])
        if closure:
            IR.immersed_closure_part(m, imm, cn, U, U[cn], NU if cn != "c" else KAPPA, want)
        got = model.tendency(n).parent()
        assert np.array_equal(got, want), (cn, np.abs(got - want).max(), np.argwhere(got != want)[:4])
        assert np.abs(want).max() > 0
    model.close()


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("case", PATH2 + tuple(IC.TILE_CASES))
def test_path_2_is_path_1(ocn, arch, tendency_impl, case, timestepper):
    """the two tendency paths give the same bits: Gⁿ, G⁻, every field and pNHS after 2 steps of a model with FPlane, ScalarDiffusivity and
    two tracers -- on the small grids and across the tile seams of T1 .. T6"""
    models = []
    for path in (1, 2):
        tendency_impl(2 if path == 2 else 0)
        ibg = IC.immersed_grid(ocn, arch, case)
        model = _model(ocn, ibg, tracers=("b", "S"), timestepper=timestepper, coriolis=ocn.FPlane(f=FCOR),
                       closure=ocn.ScalarDiffusivity(ν=NU, κ={"b": KAPPA, "S": 1e-3}))
        assert model.get_option("immersed_tendency_path") == path
        vals = smooth_state({("T" if n == "b" else n): ibg.nodes(f.loc) for n, f in model.fields().items()}, 19)
        vals["b"] = vals.pop("T")
        ocn.set_model(model, **vals)
        for _ in range(2):
            ocn.time_step(model, 0.05 / ibg.Nx)
        models.append(model)
    one, two = models
    for n in one.fields():
        assert np.array_equal(one.fields()[n].parent(), two.fields()[n].parent()), n
        assert np.array_equal(one.tendency(n).parent(), two.tendency(n).parent()), "Gⁿ " + n
        assert np.array_equal(one.tendency(n, previous=True).parent(), two.tendency(n, previous=True).parent()), "G⁻ " + n
    assert np.array_equal(one.pressures.pNHS.parent(), two.pressures.pNHS.parent()) and np.abs(one.tendency("u").parent()).max() > 0
    for model in models:
        model.close()


def test_raw_tendencies_on_path_2(ocn, arch):
    """ocn_compute_tendencies on G1 with random parent arrays (both upwind directions everywhere, transports on the walls) takes the
    flux-sharing kernel under the default tendency_impl and == the restatement; parent entries outside the range keep their bits"""
    _raw_call_is_the_restatement(ocn, IC.immersed_grid(ocn, arch, "G1"), "G1")


def _raw_fields(ocn, ibg):
    """u, v, w and two tracers with random parent arrays P, tendency fields pre-filled with random parent arrays G0"""
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField, "d": ocn.CenterField}
    f, P, G, G0 = {}, {}, {}, {}
    for q, n in enumerate("uvwcd"):
        f[n], G[n] = make[n](ibg), make[n](ibg)
        P[n] = np.asfortranarray(np.random.default_rng(70 + q).standard_normal(f[n].shape))
        G0[n] = np.asfortranarray(np.random.default_rng(80 + q).standard_normal(f[n].shape))
        f[n].set_parent(P[n])
        G[n].set_parent(G0[n])
    return f, P, G, G0


def _raw_want(ocn, case, P, G0, rng=None):
    """the restatement's answer to the raw call on _raw_fields over the range rng, computed once per (case, range) and left alone"""
    key = ("raw", case, rng)
    if key not in _shared:
        imm = _restatement(ocn, case)
        _shared[key] = {n: IR.advective_tendency(imm.m, imm, n if n in "uvw" else "c", (P["u"], P["v"], P["w"]), P[n], rng=rng, G=G0[n].copy(order="F"))
                        for n in "uvwcd"}
    return _shared[key]


def _raw_call_is_the_restatement(ocn, ibg, case, rng=None, settings=((None, None),)):
    """ocn_compute_tendencies over rng == the restatement over the whole parent array of u, v, w, c, d, once per (set, value) of settings"""
    f, P, G, G0 = _raw_fields(ocn, ibg)
    want = _raw_want(ocn, case, P, G0, rng)
    for set_, value in settings:
        if set_ is not None:
            set_(value)
        for n in "uvwcd":
            G[n].set_parent(G0[n])
        ocn.kernels.compute_tendencies(ibg, f["u"], f["v"], f["w"], [f["c"], f["d"]], G["u"], G["v"], G["w"], [G["c"], G["d"]], kernel_parameters=rng)
        for n in "uvwcd":
            got = G[n].parent()
            assert np.array_equal(got, want[n]), (case, rng, value, n, "at (i, j, k)", np.argwhere(got != want[n])[:4] - np.array(ibg.halo_size) + 1)
            assert not np.array_equal(want[n], G0[n])


@pytest.mark.parametrize("impl", [2, 0], ids=["path2", "path1"])
@pytest.mark.parametrize("case", list(IC.TILE_CASES))
def test_raw_tendencies_across_tile_edges(ocn, arch, tendency_impl, case, impl):
    """ocn_compute_tendencies with two tracers on random parent arrays on the tile-edge cases, by the flux-sharing kernel (tendency_impl 2)
    and by the per-field kernels (0): each == the restatement over the whole parent array, entries outside the range keep their bits. Where
    only path 2 fails the tile logic is at fault; where both do, the tables or the restatement. The raw entry has no report key: a model
    with two tracers on the same grid answers which path the setting takes."""
    tendency_impl(impl)
    ibg = IC.immersed_grid(ocn, arch, case)
    model = _model(ocn, ibg, tracers=("c", "d"))
    assert model.get_option("immersed_tendency_path") == (2 if impl == 2 else 1)
    model.close()
    _raw_call_is_the_restatement(ocn, ibg, case)


TRIMMED = [(3, 127, 2, 13, 2, 4),          # tiles start at i0 = 3: seams at i = 67 and j = 9
           (2, 65, 3, 9, 1, 5),            # exactly one 64 x 7 tile: its closing faces i1 + 1, j1 + 1 come from the edge wave alone
           (66, 129, 9, 15, 1, 5)]         # one tile that ends on the periodic edge in x and in y


@pytest.mark.parametrize("rng", TRIMMED, ids=["-".join(map(str, r)) for r in TRIMMED])
def test_trimmed_ranges_across_tile_edges(ocn, arch, rng):
    """kernel_parameters on T2 (129 x 15 x 5) by the flux-sharing kernel: the tiles, the edge lines and the clamp of the flag index follow
    the range, not the grid; every field takes the range as it is (no exclude_periphery)"""
    _raw_call_is_the_restatement(ocn, IC.immersed_grid(ocn, arch, "T2"), "T2", rng=rng)


@pytest.mark.parametrize("case", ["T1", "T5"])
def test_chunk_lengths_across_tile_edges(ocn, arch, role_kchunk, case):
    """every chunk length of option_variants.chunk_lengths under the immersed instantiation: the flag reads while the z-window is primed
    and in the peeled plane kc1 + 1 of every chunk, on T1 (Nz = 6, Bounded) and T5 (Nz = 9, Periodic)"""
    from option_variants import chunk_lengths
    lengths = tuple(dict.fromkeys(chunk_lengths(IC.TILE_CASES[case]["size"][2])))
    assert len(lengths) >= 7
    _raw_call_is_the_restatement(ocn, IC.immersed_grid(ocn, arch, case), case, settings=[(role_kchunk, kc) for kc in lengths])


def test_raw_entry_points_honour_the_boundary(ocn, arch):
    """ocn_compute_tendencies, ocn_compute_advective_tendency (accumulate 0 / 1), ocn_compute_closure_tendencies, ocn_add_fplane_coriolis
    and ocn_mask_immersed_field on random parent arrays on G2 (walls, a block on a wall, an isolated cell) == the restatement"""
    ibg = IC.immersed_grid(ocn, arch, "G2")
    imm = _restatement(ocn, "G2")
    m = imm.m
    rng = np.random.default_rng(5)
    make = {"u": ocn.XFaceField, "v": ocn.YFaceField, "w": ocn.ZFaceField, "c": ocn.CenterField}

    def fields(seed):
        out, parents = {}, {}
        for n in "uvwc":
            out[n] = make[n](ibg)
            parents[n] = np.asfortranarray(np.random.default_rng(seed + ord(n)).standard_normal(out[n].shape))
            out[n].set_parent(parents[n])
        return out, parents

    f, P = fields(1)
    G, G0 = fields(2)
    adv = (P["u"], P["v"], P["w"])
    ocn.kernels.compute_tendencies(ibg, f["u"], f["v"], f["w"], [f["c"]], G["u"], G["v"], G["w"], [G["c"]])
    for n in "uvwc":
        want = IR.advective_tendency(m, imm, n, adv, P[n], G=G0[n].copy(order="F"))
        assert np.array_equal(G[n].parent(), want), n
    a, A = fields(3)
    for n in "uvwc":
        for accumulate in (False, True):
            H, H0 = fields(4)
            ocn.kernels.compute_advective_tendency(ibg, a["u"], a["v"], a["w"], f[n], n, H[n], accumulate=accumulate)
            want = IR.advective_tendency(m, imm, n, (A["u"], A["v"], A["w"]), P[n], G=H0[n].copy(order="F"), accumulate=accumulate)
            assert np.array_equal(H[n].parent(), want), (n, accumulate)
    closure = ocn.ScalarDiffusivity(ν=NU, κ=KAPPA)
    H, H0 = fields(6)
    ocn.kernels.compute_closure_tendencies(ibg, [f[n] for n in "uvwc"], [H[n] for n in "uvwc"], closure, ("c",))
    for n in "uvwc":
        want = IR.immersed_closure_part(m, imm, n, P, P[n], NU if n != "c" else KAPPA, H0[n].copy(order="F"))
        assert np.array_equal(H[n].parent(), want), n
    H, H0 = fields(8)
    ocn.kernels.add_fplane_coriolis(ibg, FCOR, f["u"], f["v"], H["u"], H["v"])
    Gu, Gv = H0["u"].copy(order="F"), H0["v"].copy(order="F")
    IR.fplane(m, imm, FCOR, P, Gu, Gv)
    assert np.array_equal(H["u"].parent(), Gu) and np.array_equal(H["v"].parent(), Gv)
    for n in "uvwc":
        ocn.mask_immersed_field(f[n], -3.5)
        assert np.array_equal(f[n].parent(), imm.mask_field(P[n].copy(order="F"), R.LOCS[n], -3.5)) and (f[n].parent() == -3.5).any()
    # a field on a plain grid is left alone (the fallback of mask_immersed_field.jl:46)
    plain = ocn.CenterField(IC.underlying_grid(ocn, arch, "G2"))
    plain.set_parent(P["c"])
    ocn.mask_immersed_field(plain, -3.5)
    assert np.array_equal(plain.parent(), P["c"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. an empty boundary is the plain model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("case", ["G1", "G2", "G3"])
def test_empty_boundary_is_the_plain_model(ocn, arch, case, timestepper):
    """with the bottom below the domain nothing is immersed: the order table reproduces outside_*_halo at the walls, no flux is masked, the
    masks write nothing -- every field and pNHS equal the plain model's on the same grid at the same halo after 3 steps, bit for bit,
    although the plain model composes its step from the flux-sharing kernels, the epilogue and the folded substeps"""
    models = []
    for immersed in (True, False):
        grid = IC.immersed_grid(ocn, arch, case, IC.EMPTY) if immersed else IC.underlying_grid(ocn, arch, case)
        model = _model(ocn, grid, tracers=("b", "S"), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=FCOR),
                       closure=ocn.ScalarDiffusivity(ν=NU, κ={"b": KAPPA, "S": 1e-3}))
        assert model.get_option("immersed") == int(immersed)
        vals = smooth_state({("T" if n == "b" else n): grid.nodes(f.loc) for n, f in model.fields().items()}, 21)
        vals["b"] = vals.pop("T")
        ocn.set_model(model, **vals)
        for _ in range(3):
            ocn.time_step(model, 0.05 / grid.Nx)
        models.append(model)
    a, b = models
    assert not _core(_restatement(ocn, case, IC.EMPTY).m, a.grid.immersed_cell_mask()).any()
    for n in a.fields():
        assert np.array_equal(a.fields()[n].parent(), b.fields()[n].parent()), n
        assert np.array_equal(a.tendency(n).parent(), b.tendency(n).parent()), "G " + n
    assert np.array_equal(a.pressures.pNHS.parent(), b.pressures.pNHS.parent())
    assert a.clock.time == b.clock.time and np.abs(a.velocities.u.parent()).max() > 0
    for model in models:
        model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the model against the orchestrated yardstick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("case", [c for c in IC.CASES if c != "G5"])            # (G5 has no top: test_triply_periodic_model_is_the_yardstick)
def test_model_is_the_orchestrated_yardstick(ocn, oracle, arch, case, timestepper):
    """3 steps at Δt = 0.05 / Nx with BuoyancyTracer, FPlane, ScalarDiffusivity, an array forcing on S and a Flux condition on b's top:
    fields rel_err < 1e-12 over the interior, immersed cells included; pNHS to 1e-12 of the scale of
    test_gpu_vertically_implicit.test_model_is_the_orchestrated_yardstick; the clock `==`; tracers exactly 0 at their immersed nodes after
    update_state!. The velocity mask is seen directly only where it is the last thing to run, in set! without the projection (the mask of
    ocn_model_set_finalize); the one at the head of the pressure step is covered through the comparison with the yardstick, which has it
    (a build without it fails this test on every grid)."""
    _model_is_the_orchestrated_yardstick(ocn, oracle, arch, case, timestepper, 3)


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_tile_model_is_the_orchestrated_yardstick(ocn, oracle, arch, timestepper):
    """the same physics on T1 (65 x 8 x 6: two x tiles, two row tiles, the edge wave live) for one step -- three RK3 stages, or AB2's
    forward-Euler first step -- with the same bounds and the same exact zeros"""
    _model_is_the_orchestrated_yardstick(ocn, oracle, arch, "T1", timestepper, 1)


def _model_is_the_orchestrated_yardstick(ocn, oracle, arch, case, timestepper, steps):
    ibg = IC.immersed_grid(ocn, arch, case)
    g = IC.oracle_grid(oracle, case)
    imm = _restatement(ocn, case)
    m = imm.m
    forcing = 0.1 * np.random.default_rng(4).standard_normal(ibg.size)
    F = ocn.FieldBoundaryConditions
    model = _model(ocn, ibg, tracers=("b", "S"), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=FCOR),
                   closure=ocn.ScalarDiffusivity(ν=NU, κ={"b": KAPPA, "S": 1e-3}), forcing={"S": forcing},
                   boundary_conditions={"b": F(top=ocn.FluxBoundaryCondition(0.03))})
    assert model.get_option("immersed_tendency_path") == (2 if case in PATH2 + tuple(IC.TILE_CASES) else 1) and model.get_option("forcing_path") == 3
    yard = IR.ImmersedOrchestrated(oracle, g, 2, NU, (KAPPA, 1e-3), imm.cell, buoyancy_index=0, fcor=FCOR, forcing={"c1": forcing},
                                   bcs={"c0": {"top": ("flux", 0.03)}})
    vals = smooth_state({("T" if n == "b" else n): ibg.nodes(f.loc) for n, f in model.fields().items()}, 17)
    vals["b"] = vals.pop("T")
    # the velocity mask alone: set! without the projection leaves exact zeros at the immersed peripheral nodes of each velocity
    ocn.set_model(model, enforce_incompressibility=False, **vals)
    for n in "uvw":
        I, J, K = (np.arange(1, s + 1).reshape([-1 if q == d else 1 for q in range(3)]) for d, s in enumerate(m.N))
        masked = np.broadcast_to(imm.bit(R.LOCS[n], I, J, K), m.N)
        inner = model.fields()[n].parent()[tuple(slice(h, h + s) for h, s in zip(m.H, m.N))]
        assert masked.any() and np.all(inner[masked] == 0.0) and np.abs(inner[~masked]).max() > 0, n
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["b"], c1=vals["S"])
    dt = 0.05 / ibg.Nx
    for _ in range(steps):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    cells = _core(m, imm.cell)
    for gn, cn in zip(("u", "v", "w", "b", "S"), yard.names):
        a, b = _core(m, model.fields()[gn].parent()), _core(m, yard.U[cn])
        assert np.all(np.isfinite(a))
        print(f"{case} {timestepper} {gn}: rel_err {rel_err(a, b):.3e}")
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
        if cn.startswith("c"):
            assert np.all(a[cells] == 0.0)
    a, b = _core(m, model.pressures.pNHS.parent()), _core(m, yard.p)
    spacing = max(d for d, t in zip((ibg.Δxᶜᵃᵃ, ibg.Δyᵃᶜᵃ), ibg.topology) if t is not ocn.Flat)
    pscale = max(np.abs(b).max(), umax * spacing / dt)
    print(f"{case} {timestepper} p: max abs difference {np.max(np.abs(a - b)):.3e} on the scale {pscale:.3e}")
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration == steps
    assert model.clock.last_Δt == yard.last_dt and model.clock.last_stage_Δt == yard.last_stage_dt
    # at the end of a step the velocities at immersed faces are NOT zero: they carry -Δt ∂p until the next mask (the reference's behaviour)
    w_faces = np.broadcast_to(imm.bit(R.LOCS["w"], *(np.arange(1, s + 1).reshape([-1 if q == d else 1 for q in range(3)]) for d, s in enumerate(m.N))), m.N)
    assert np.abs(model.velocities.w.parent()[tuple(slice(h, h + s) for h, s in zip(m.H, m.N))][w_faces]).max() > 0
    model.close()


def _compare(case, label, model, yard, names, m, dt, spacing):
    umax = max(np.abs(yard.U[n]).max() for n in "uvw")
    for gn, cn in zip(names, yard.names):
        a, b = _core(m, model.fields()[gn].parent()), _core(m, yard.U[cn])
        assert np.all(np.isfinite(a))
        print(f"{case} {label} {gn}: rel_err {rel_err(a, b):.3e}")
        assert rel_err(a, b) < 1e-12, (gn, rel_err(a, b))
    a, b = _core(m, model.pressures.pNHS.parent()), _core(m, yard.p)
    pscale = max(np.abs(b).max(), umax * spacing / dt)
    print(f"{case} {label} p: max abs difference {np.max(np.abs(a - b)):.3e} on the scale {pscale:.3e}")
    assert np.max(np.abs(a - b)) < 1e-12 * pscale
    assert model.clock.time == yard.time and model.clock.iteration == yard.iteration


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_triply_periodic_model_is_the_yardstick(ocn, oracle, arch, timestepper):
    """G5, (Periodic, Periodic, Periodic) with immersed cells that are neighbours across every wrap: the pressure step's source term and
    correction read wrapped interior indices right after the velocity mask, and nothing of the plain triply periodic step is folded
    (halo_fill_folded and stage1_source_fused answer 0). FPlane, ScalarDiffusivity, an array forcing; 3 steps to 1e-12."""
    ibg = IC.immersed_grid(ocn, arch, "G5")
    g = IC.oracle_grid(oracle, "G5")
    imm = _restatement(ocn, "G5")
    forcing = 0.1 * np.random.default_rng(8).standard_normal(ibg.size)
    model = _model(ocn, ibg, tracers=("c",), timestepper=timestepper, coriolis=ocn.FPlane(f=FCOR), closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA),
                   forcing={"c": forcing})
    yard = IR.ImmersedOrchestrated(oracle, g, 1, NU, (KAPPA,), imm.cell, fcor=FCOR, forcing={"c0": forcing})
    vals = smooth_state({("T" if n == "c" else n): ibg.nodes(f.loc) for n, f in model.fields().items()}, 31)
    vals["c"] = vals.pop("T")
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["c"])
    dt = 0.05 / ibg.Nx
    for _ in range(3):
        ocn.time_step(model, dt)
        yard.time_step(dt) if timestepper == "RungeKutta3" else yard.time_step_ab2(dt)
    assert model.get_option("halo_fill_folded") == 0 and model.get_option("stage1_source_fused") == 0
    _compare("G5", timestepper, model, yard, ("u", "v", "w", "c"), imm.m, dt, max(ibg.Δxᶜᵃᵃ, ibg.Δyᵃᶜᵃ))
    model.close()


def test_seawater_wall_conditions_and_a_function_flux(ocn, oracle, arch):
    """G1 with SeawaterBuoyancy(LinearEquationOfState), a Value condition on T's top, a Gradient condition on T's bottom and a Flux condition
    on S's top that is a FUNCTION of (x, y, t), recorded and evaluated on the device: 2 RK3 steps against the yardstick, which takes the
    function's values at the nodes as an array, to 1e-12"""
    ibg = IC.immersed_grid(ocn, arch, "G1")
    g = IC.oracle_grid(oracle, "G1")
    imm = _restatement(ocn, "G1")
    F = ocn.FieldBoundaryConditions
    grav, alpha, beta = 9.80665, 2e-4, 8e-4
    flux = lambda x, y, t: 0.02 + 0.05 * x * (1.0 - x) + 0.01 * y          # noqa: E731
    model = _model(ocn, ibg, tracers=("T", "S"), closure=ocn.ScalarDiffusivity(ν=NU, κ={"T": KAPPA, "S": 1e-3}),
                   buoyancy=ocn.SeawaterBuoyancy(gravitational_acceleration=grav,
                                                 equation_of_state=ocn.LinearEquationOfState(thermal_expansion=alpha, haline_contraction=beta)),
                   boundary_conditions={"T": F(top=ocn.ValueBoundaryCondition(0.4), bottom=ocn.GradientBoundaryCondition(0.1)),
                                        "S": F(top=ocn.FluxBoundaryCondition(flux))})
    assert model.get_option("boundary_functions") == 1
    x, y, _ = ibg.nodes((ocn.Center,) * 3)
    values = np.asfortranarray(np.broadcast_to(flux(x, y, 0.0)[:, :, 0], (ibg.Nx, ibg.Ny)))
    yard = IR.ImmersedOrchestrated(oracle, g, 2, NU, (KAPPA, 1e-3), imm.cell, seawater=(grav, alpha, beta),
                                   bcs={"c0": {"top": ("value", 0.4), "bottom": ("gradient", 0.1)}, "c1": {"top": ("flux", values)}})
    vals = smooth_state({n: ibg.nodes(f.loc) for n, f in model.fields().items()}, 23)
    ocn.set_model(model, **vals)
    yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["T"], c1=vals["S"])
    dt = 0.05 / ibg.Nx
    for _ in range(2):
        ocn.time_step(model, dt)
        yard.time_step(dt)
    assert np.array_equal(model.boundary_function_values("S", "top"), values)
    _compare("G1", "seawater", model, yard, ("u", "v", "w", "T", "S"), imm.m, dt, max(ibg.Δxᶜᵃᵃ, ibg.Δyᵃᶜᵃ))
    model.close()


def test_forcing_program_wizard_and_simulation(ocn, arch):
    """on G1: a Relaxation whose mask is a function of the user's (a forcing program evaluated in the volume) gives what the same mask as a
    GaussianMask gives, to 1e-12; cell_advection_timescale is the plain grid's expression of the model's velocities; a Simulation with a
    TimeStepWizard callback runs to its stop_iteration with finite fields and tracers that stay 0 in the solid"""
    ibg = IC.immersed_grid(ocn, arch, "G1")
    imm = _restatement(ocn, "G1")
    m = imm.m
    models = []
    for mask in (ocn.GaussianMask("z", center=-0.2, width=0.1), lambda x, y, z: ocn.exp(-((z + 0.2) * (z + 0.2)) / (2 * (0.1 * 0.1)))):
        model = _model(ocn, ibg, tracers=("b",), buoyancy=ocn.BuoyancyTracer(), closure=ocn.ScalarDiffusivity(ν=NU, κ=KAPPA),
                       forcing={"b": ocn.Relaxation(rate=0.8, mask=mask, target=0.3)})
        ocn.set_model(model, **_state(ibg, model, 13))
        models.append(model)
    builtin, program = models
    assert program.get_option("forcing_functions") == 1 and builtin.get_option("forcing_functions") == 0
    for _ in range(2):
        for model in models:
            ocn.time_step(model, 0.05 / ibg.Nx)
    for n in builtin.fields():
        a, b = _core(m, program.fields()[n].parent()), _core(m, builtin.fields()[n].parent())
        assert rel_err(a, b) < 1e-12, (n, rel_err(a, b))
    builtin.close()
    model = program
    u, v, w = (_core(m, model.fields()[n].parent()) for n in "uvw")
    Nx, Ny, Nz = m.N
    dzf = m.dzf[m.H[2]:m.H[2] + Nz][None, None, :]
    rate = np.abs(u[:Nx, :Ny, :Nz]) / m.dx + np.abs(v[:Nx, :Ny, :Nz]) / m.dy + np.abs(w[:Nx, :Ny, :Nz]) / dzf
    tau = ocn.cell_advection_timescale(model)
    assert abs(tau - 1.0 / rate.max()) <= 1e-12 * tau
    sim = ocn.Simulation(model, Δt=0.05 / ibg.Nx, stop_iteration=model.clock.iteration + 3)
    sim.callbacks["wizard"] = ocn.Callback(ocn.TimeStepWizard(cfl=0.3, max_change=1.5), ocn.IterationInterval(1))
    ocn.run(sim)
    assert model.clock.iteration == 5 and np.isfinite(sim.Δt) and sim.Δt > 0
    assert all(np.isfinite(f.parent()).all() for f in model.fields().values())
    assert np.all(_core(m, model.tracers.b.parent())[_core(m, imm.cell)] == 0.0)
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. no flux through the solid
# ---------------------------------------------------------------------------------------------------------------------
def test_no_flux_through_the_solid(ocn, oracle, arch):
    """G1, velocities zero, κ > 0, a tracer blob beside the bump, 20 AB2 steps: Σ c V over the active cells drifts by no more than 8 x the
    drift of the numpy yardstick in the same run (the margin DESIGN.md 3.1 uses for round-off against a yardstick), and the blob has
    reached the solid. Measured on the MI355X: device drift 8.674e-19, yardstick drift 8.674e-19 of a content of 3.975718e-03."""
    ibg = IC.immersed_grid(ocn, arch, "G1")
    g = IC.oracle_grid(oracle, "G1")
    imm = _restatement(ocn, "G1")
    m = imm.m
    kappa = 0.02
    model = _model(ocn, ibg, tracers=("c",), timestepper="QuasiAdamsBashforth2", closure=ocn.ScalarDiffusivity(ν=0.0, κ=kappa))
    yard = IR.ImmersedOrchestrated(oracle, g, 1, 0.0, (kappa,), imm.cell)
    x, y, z = ibg.nodes((ocn.Center,) * 3)
    blob = np.exp(-((x - 0.45) ** 2 + (y - 0.1) ** 2 + (z + 0.75) ** 2) / 0.01)          # over the trench, between the two columns of five
    ocn.set_model(model, c=blob)
    yard.set(c0=blob)
    volume = (m.dx * m.dy) * m.dzc[m.H[2]:m.H[2] + m.N[2]][None, None, :]
    active = ~_core(m, imm.cell)
    content = lambda a: float(np.sum((_core(m, a) * volume)[active]))                     # noqa: E731
    before = content(model.tracers.c.parent())
    assert before == content(yard.U["c0"]) and before > 0
    beside = np.zeros(m.N, dtype=bool)                                                     # active cells with an immersed neighbour
    cells = _core(m, imm.cell)
    for d in range(3):
        for s in (1, -1):
            beside |= np.roll(cells, s, axis=d) & ~cells
    dt = 0.1 * float(np.min(m.dzc)) ** 2 / kappa
    for _ in range(20):
        ocn.time_step(model, dt)
        yard.time_step_ab2(dt)
    c = _core(m, model.tracers.c.parent())
    drift, yard_drift = abs(content(model.tracers.c.parent()) - before), abs(content(yard.U["c0"]) - before)
    print(f"tracer content {before:.6e}: device drift {drift:.3e}, yardstick drift {yard_drift:.3e}")
    assert np.abs(c[beside]).max() > 1e-3 * np.abs(c).max()                                # the blob is at the wall
    assert np.all(c[cells] == 0.0)
    assert drift <= 8 * yard_drift
    assert rel_err(c, _core(m, yard.U["c0"])) < 1e-12
    model.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the reference's Gaussian immersed diffusion
# ---------------------------------------------------------------------------------------------------------------------
def test_gaussian_immersed_diffusion(ocn, arch):
    """test_immersed_diffusion (test/test_dynamics.jl:89-116) with a NonhydrostaticModel: (Flat, Flat, Bounded), Nz = 128, z in (-0.5, 0.5),
    κ = 1, a bottom at 0, 100 steps of 0.1 Δz² / κ: the upper half of the immersed model ≈ the full model's (isapprox, rtol = √eps) -- the
    Gaussian is even about the bottom, where the full model therefore has no flux either"""
    Nz = 128
    topology = (ocn.Flat, ocn.Flat, ocn.Bounded)
    full_grid = ocn.RectilinearGrid(arch, size=Nz, z=(-0.5, 0.5), topology=topology)
    ibg = ocn.ImmersedBoundaryGrid(ocn.RectilinearGrid(arch, size=Nz, z=(-0.5, 0.5), topology=topology, halo=4), ocn.GridFittedBottom(0.0))
    closure = ocn.ScalarDiffusivity(κ=1.0)
    results = []
    for grid in (full_grid, ibg):
        model = _model(ocn, grid, tracers=("c",), closure=closure)
        ocn.set_model(model, c=lambda x, y, z: np.exp(-z ** 2 / 0.02) + 0 * x + 0 * y)
        dt = 0.1 * (1.0 / Nz) ** 2 / 1.0
        for _ in range(100):
            ocn.time_step(model, dt)
        results.append(model.tracers.c.interior()[0, 0, Nz // 2:].copy())
        model.close()
    c_full, c_immersed = results
    rtol = np.sqrt(np.finfo(np.float64).eps)
    assert np.all(np.abs(c_full - c_immersed) <= rtol * np.maximum(np.abs(c_full), np.abs(c_immersed)))
    assert c_full.max() < 0.99 and c_full.max() > 0.5                                      # it has diffused, and is still there


# ---------------------------------------------------------------------------------------------------------------------
# 7. the answers of the new entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_answers(ocn, arch):
    L = ocn._lib.lib()
    OK, EINVAL, ENOTSUP, ESTATE = 0, -1, -2, -3
    ub = C.POINTER(C.c_ubyte)
    # a plain grid has no flags; masking a field on it does nothing
    plain = IC.underlying_grid(ocn, arch, "G1")
    assert L.ocn_grid_get_immersed_flags(plain.handle, None, None) == ESTATE
    # a halo of the buffer only is refused: an immersed grid needs buffer + 1
    small = IC.underlying_grid(ocn, arch, "G1", halo=(3, 3, 3))
    cell = np.zeros(small.total_size((ocn.Center,) * 3), dtype=np.uint8, order="F")
    assert L.ocn_grid_set_immersed_boundary(small.handle, cell.ctypes.data_as(ub)) == EINVAL and b"buffer + 1" in L.ocn_last_error()
    # set, read, clear
    cell = np.asfortranarray(_restatement(ocn, "G1").cell, dtype=np.uint8)
    assert L.ocn_grid_set_immersed_boundary(plain.handle, cell.ctypes.data_as(ub)) == OK
    periphery = np.empty(cell.shape, dtype=np.uint8, order="F")
    assert L.ocn_grid_get_immersed_flags(plain.handle, periphery.ctypes.data_as(ub), None) == OK
    assert np.array_equal(periphery, _restatement(ocn, "G1").periphery)
    assert L.ocn_grid_set_immersed_boundary(plain.handle, None) == OK and L.ocn_grid_get_immersed_flags(plain.handle, None, None) == ESTATE
    # the boundary may not change under a model
    ibg = IC.immersed_grid(ocn, arch, "G1")
    model = _model(ocn, ibg, tracers=("b",))
    assert L.ocn_grid_set_immersed_boundary(ibg.handle, cell.ctypes.data_as(ub)) == ESTATE
    assert L.ocn_grid_set_immersed_boundary(ibg.handle, None) == ESTATE
    # what an immersed grid does not serve answers OCN_ENOTSUP and names the grid
    h = model.handle
    one = (C.c_double * 1)(1e-3)
    for status in (L.ocn_model_set_vertically_implicit(h, 1), L.ocn_model_set_amd(h, 1 / 3, one), L.ocn_model_set_smagorinsky(h, 0.16, 1.0, 0, one),
                   L.ocn_model_set_cartesian_coriolis(h, 1, 0.0, 0.1, 1.0), L.ocn_model_set_gravity_unit_vector(h, 1, 0.0, 0.1, -0.99),
                   L.ocn_model_set_background_field(h, b"u", model.velocities.u.data),
                   L.ocn_model_set_open_boundary_scheme(h, b"w", 5, 1, 0.0, 1.0)):
        assert status == ENOTSUP and b"ImmersedBoundaryGrid" in L.ocn_last_error(), L.ocn_last_error()
    u, v, w, b = model.velocities.u, model.velocities.v, model.velocities.w, model.tracers.b
    with pytest.raises(ocn.OcnError, match="ImmersedBoundaryGrid"):
        ocn.kernels.compute_closure_tendencies_vertically_implicit(ibg, [u, v, w, b], [model.tendency(n) for n in ("u", "v", "w", "b")],
                                                                   ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=1e-3, κ=1e-3), ("b",))
    with pytest.raises(ocn.OcnError, match="ImmersedBoundaryGrid"):
        ocn.kernels.implicit_step(ibg, b, 1e-3, 0.1)
    operand = ocn._lib.Operand()
    out = ocn.CenterField(ibg)
    assert L.ocn_compute_operation(ibg.handle, C.byref(operand), out.data) == ENOTSUP and b"ImmersedBoundaryGrid" in L.ocn_last_error()
    model.close()
    # ... and once the model is gone the boundary may change again
    assert L.ocn_grid_set_immersed_boundary(ibg.handle, cell.ctypes.data_as(ub)) == OK
