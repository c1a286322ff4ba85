"""GPU: the pressure step of a triply periodic model with its neighbouring passes folded in (ocn_api.hip: pressure_step).

  * fused_halo = 1: the correction kernel writes every periodic image of the cell it corrects -- u, v, w, the stored pNHS and the tracers --
    so no fill_halo_regions! launch is left in a time-step ("halo_fill_folded" reads 1);
  * fuse_substep = 1: the first RK3 substep rides in the source-term and correction kernels ("stage1_source_fused" reads 1).

Shapes: (3, 8, 8) has Nx = H, every cell has two x images; (5, 8, 8) has H < Nx < 2H, some cells have images on both sides; (70, 16, 8) has a
ragged second 64-wide block; (64, 8, 16). The split solver needs Ny = 2^m >= 8 and the fused z transform Nz = 2^m. Tracer counts 0, 2, 3.
No tolerance is new: bit-identity with the separate kernels, helpers.rel_err < 1e-12 against the oracle, pNHS with the error model of
test_gpu_option_variants.py."""
import numpy as np
import pytest

from helpers import smooth_state
from test_gpu_option_variants import _assert_within_1e12_of_the_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8, 8), (5, 8, 8), (70, 16, 8), (64, 8, 16)]
NTRACERS = [0, 2, 3]
CASES = [(s, n) for s in SHAPES for n in NTRACERS]
TRACERS = ("T", "S", "C3")
CNAMES = ["u", "v", "w", "c0", "c1", "c2"]
SEPARATE = {"fused_halo": 0, "fuse_substep": 0}
H = 3
_cache = {}


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else "ntr%d" % v


def _grid(ocn, arch, size):
    if ("grid", size) not in _cache:
        _cache["grid", size] = ocn.RectilinearGrid(arch, size=size, extent=(1, 1, 1))
    return _cache["grid", size]


def _dt(grid):
    return 0.1 * min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ) / 0.6


def _values(grid, model, seed):
    return smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed)


def _state_of(model):
    out = {n: f.parent() for n, f in model.fields().items()}
    out["pNHS"] = model.pressures.pNHS.parent()
    return out


def _model(ocn, grid, ntr, opts):
    """a model with the options; asserts the path facts of every case: the fused z transform runs (so the split dense-solution path does)"""
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=TRACERS[:ntr])
    for k, v in opts.items():
        model.set_option(k, v)
    assert model.get_option("fused_zfft_active") == 1
    return model


def _assert_path(model, folded):
    assert model.get_option("halo_fill_folded") == folded and model.get_option("stage1_source_fused") == folded, \
        (folded, model.get_option("halo_fill_folded"), model.get_option("stage1_source_fused"))


def _run(ocn, arch, size, ntr, opts, folded):
    """smooth_state(1234); the states after 1, 3 and 5 RK3 steps; a second model takes two steps, a set_model with new values (seed 77) and one
    more step -> [after 1, after 3, after 5, after 2 + set_model + 1]"""
    key = ("run", size, ntr, folded)
    if key not in _cache:
        grid = _grid(ocn, arch, size)
        model = _model(ocn, grid, ntr, opts)
        ocn.set_model(model, **_values(grid, model, 1234))
        out = []
        for step in range(5):
            ocn.time_step(model, _dt(grid))
            _assert_path(model, folded)
            if step % 2 == 0:
                out.append(_state_of(model))
        model.close()
        model = _model(ocn, grid, ntr, opts)
        ocn.set_model(model, **_values(grid, model, 1234))
        for _ in range(2):
            ocn.time_step(model, _dt(grid))
        ocn.set_model(model, **_values(grid, model, 77))
        ocn.time_step(model, _dt(grid))
        _assert_path(model, folded)
        out.append(_state_of(model))
        model.close()
        _cache[key] = out
    return _cache[key]


def _folded(ocn, arch, size, ntr):
    return _run(ocn, arch, size, ntr, {}, 1)


def _separate(ocn, arch, size, ntr):
    return _run(ocn, arch, size, ntr, SEPARATE, 0)


def _assert_halos_wrap(state, tag):
    for n, a in state.items():
        interior = a[H:-H, H:-H, H:-H]
        assert np.abs(interior).max() > 0, (tag, n)
        want = np.pad(interior, H, mode="wrap")
        assert np.array_equal(a, want), (tag, n, int((a != want).sum()))


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_halos_are_the_wrapped_interior(ocn, arch, size, ntr):
    """after 1 and after 3 steps every parent array -- u, v, w, each tracer, pNHS -- equals its interior padded periodically: the correction
    kernel wrote every image, edges and corners included (no second HIP path is needed to say so)"""
    after1, after3 = _folded(ocn, arch, size, ntr)[:2]
    _assert_halos_wrap(after1, (size, ntr, "1 step"))
    _assert_halos_wrap(after3, (size, ntr, "3 steps"))


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_three_steps_against_the_oracle(ocn, oracle, arch, size, ntr):
    grid = _grid(ocn, arch, size)
    names = ["u", "v", "w"] + list(TRACERS[:ntr])
    locs = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face)}
    vals = smooth_state({n: grid.nodes(locs.get(n, (ocn.Center,) * 3)) for n in names}, 1234)
    m_cpu = oracle.Model(oracle.Grid(size), ntr)
    m_cpu.set(**{cn: vals[n] for cn, n in zip(CNAMES, names)})
    for _ in range(3):
        m_cpu.time_step(_dt(grid))
    ref = {n: m_cpu.field(cn).copy() for cn, n in zip(CNAMES, names)} | {"pNHS": m_cpu.field("p").copy()}
    _assert_within_1e12_of_the_oracle(_folded(ocn, arch, size, ntr)[1], ref, grid, _dt(grid), (size, ntr))


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_bit_identical_to_the_separate_kernels(ocn, arch, size, ntr):
    """fused_halo = 0, fuse_substep = 0: fill_periodic_xyz_kernel x 3 per fill, rk3_substep_kernel + source_term_kernel, the plain correction
    kernel. Whole parent arrays after 1 and 3 steps"""
    got, want = _folded(ocn, arch, size, ntr), _separate(ocn, arch, size, ntr)
    for a, b, tag in zip(got[:2], want[:2], ("1 step", "3 steps")):
        for n in b:
            assert np.array_equal(a[n], b[n]), (size, ntr, tag, n, int((a[n] != b[n]).sum()))


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_each_fold_alone_is_bit_identical_too(ocn, arch, size, ntr):
    """the two folds are independent switches: the correction kernel has an instantiation for each alone"""
    grid = _grid(ocn, arch, size)
    want = _separate(ocn, arch, size, ntr)[1]
    for opts, facts in (({"fuse_substep": 0}, (1, 0)), ({"fused_halo": 0}, (0, 1))):
        model = _model(ocn, grid, ntr, opts)
        ocn.set_model(model, **_values(grid, model, 1234))
        for _ in range(3):
            ocn.time_step(model, _dt(grid))
        assert (model.get_option("halo_fill_folded"), model.get_option("stage1_source_fused")) == facts, opts
        state = _state_of(model)
        model.close()
        for n in want:
            assert np.array_equal(state[n], want[n]), (size, ntr, opts, n)


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_no_stale_skip_after_set_model(ocn, arch, size, ntr):
    """two steps, set_model with new values, one step: the skipped fill is a property of one time-step call, not of the model -- set_model's
    own fills run, and the step after it leaves wrapped halos and the separate kernels' bits again"""
    got, want = _folded(ocn, arch, size, ntr)[3], _separate(ocn, arch, size, ntr)[3]
    _assert_halos_wrap(got, (size, ntr, "after set_model"))
    for n in want:
        assert np.array_equal(got[n], want[n]), (size, ntr, n, int((got[n] != want[n]).sum()))
    assert any(not np.array_equal(got[n], _folded(ocn, arch, size, ntr)[1][n]) for n in got)


@pytest.mark.parametrize("size,ntr", CASES, ids=_ids)
def test_graph_replay_of_the_folded_step(ocn, arch, size, ntr):
    """use_graph = 1: the first step runs plain, the second is captured, three replays follow -- bit-identical to five plain steps"""
    grid = _grid(ocn, arch, size)
    model = _model(ocn, grid, ntr, {"use_graph": 1})
    ocn.set_model(model, **_values(grid, model, 1234))
    for _ in range(5):
        ocn.time_step(model, _dt(grid))
    _assert_path(model, 1)
    assert model.get_option("graph_failures") == 0 and model.get_option("graph_captures") == 1 and model.get_option("graph_replays") == 3
    state = _state_of(model)
    model.close()
    want = _folded(ocn, arch, size, ntr)[2]
    for n in want:
        assert np.array_equal(state[n], want[n]), (size, ntr, n)


def test_a_bounded_grid_keeps_its_launches(ocn, arch):
    """(Periodic, Periodic, Bounded): both report keys read 0 after a step"""
    grid = ocn.RectilinearGrid(arch, size=(16, 8, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    ocn.set_model(model, **_values(grid, model, 1234))
    ocn.time_step(model, _dt(grid))
    _assert_path(model, 0)
    model.close()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
