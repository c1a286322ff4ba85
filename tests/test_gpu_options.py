"""GPU: a model's tuning options are its own (include/ocn_mi355x.h: ocn_set_option) -- the library defaults are copied when a model is
created, a model's setting stays in that model, and a later library default does not reach a model that exists."""
import numpy as np
import pytest

from helpers import smooth_state

pytestmark = pytest.mark.gpu


def _state(model):
    return {n: f.parent() for n, f in model.fields().items()}


def _random_state(grid, model, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1.0, 1.0, np.broadcast(*grid.nodes(f.loc)).shape) for n, f in model.fields().items()}


def test_a_model_option_does_not_reach_another_model(ocn, arch):
    """arithmetic = 1 on model A only; A and B stepped interleaved on one grid: B's fields are bit for bit those of a model stepped alone
    with the defaults before A existed, A's are not (the contracted flux ran), B still reports 0"""
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), extent=(1, 1, 1))
    dt = 0.1 * grid.Δxᶜᵃᵃ / 0.6

    def model():
        m = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
        ocn.set_model(m, **_random_state(grid, m, 21))
        return m

    alone = model()
    for _ in range(3):
        ocn.time_step(alone, dt)
    ref = _state(alone)
    alone.close()
    a, b = model(), model()
    a.set_option("arithmetic", 1)
    for _ in range(3):
        ocn.time_step(a, dt)
        ocn.time_step(b, dt)
    assert a.get_option("arithmetic") == 1 and b.get_option("arithmetic") == 0
    for n, x in _state(b).items():
        assert np.array_equal(x, ref[n]), n
    assert any(not np.array_equal(x, ref[n]) for n, x in _state(a).items())
    a.close()
    b.close()


def test_a_library_default_reaches_only_models_created_afterwards(ocn, arch):
    """ocn_set_option("epilogue_march", 0) with a ScalarDiffusivity model alive: that model keeps 1 and steps exactly as a model that never
    saw the call; a model created afterwards starts from 0"""
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0.0, 1.0), y=(0.0, 1.0), z=(-1.0, 0.0),
                               topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    kw = dict(advection=ocn.WENO(), tracers=("T", "S"), closure=ocn.ScalarDiffusivity(ν=2e-3, κ=1e-3))

    def model():
        m = ocn.NonhydrostaticModel(grid=grid, **kw)
        ocn.set_model(m, **smooth_state({n: grid.nodes(f.loc) for n, f in m.fields().items()}, 5))
        return m

    def run(m):
        for _ in range(3):
            ocn.time_step(m, 1e-3)
        out = _state(m)
        m.close()
        return out

    ref = run(model())
    m = model()
    try:
        ocn.set_option("epilogue_march", 0)
        assert m.get_option("epilogue_march") == 1
        out = run(m)
        later = ocn.NonhydrostaticModel(grid=grid, **kw)
        assert later.get_option("epilogue_march") == 0
        later.close()
    finally:
        ocn.set_option("epilogue_march", 1)
    for n in ref:
        assert np.array_equal(out[n], ref[n]), n


def test_options_read_at_creation_are_refused_on_a_model(ocn, arch):
    """a key the solver reads only while it is built (c2r_strided) cannot change on a model that exists: OcnError, the model keeps the
    value it was created with; the partitioned step's keys are refused on a single-GPU model"""
    grid = ocn.RectilinearGrid(arch, size=(16, 16, 16), extent=(1, 1, 1))
    m = ocn.NonhydrostaticModel(grid=grid, tracers=("T",))
    with pytest.raises(ocn.OcnError, match="ocn_set_option"):
        m.set_option("c2r_strided", 0)
    assert m.get_option("c2r_strided") == 1
    with pytest.raises(ocn.OcnError):
        m.set_option("async_halos", 0)
    m.close()
