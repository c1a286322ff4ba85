"""The oracle alone on the states of value_domain_cases.py: what makes each of them a fair question to put to the GPU kernels
(tests/test_gpu_value_domain.py compares bits with the oracle, so the oracle has to be finite, non-trivial and IEEE where the kernels' fast
reciprocals leave their documented ranges). Every bound here is a condition on an INPUT: a state that misses one is changed, not the bound."""
import numpy as np
import pytest

import value_domain_cases as V

FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def tendencies(oracle):
    return {name: V.OracleTendencies(oracle, grid) for name, grid in V.GRIDS.items()}


@pytest.mark.parametrize("state,k", V.LADDER, ids=lambda p: str(p))
@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_the_oracle_is_finite_on_every_rung(tendencies, grid, state, k):
    G = tendencies[grid](V.state_of(V.GRIDS[grid], state, k))
    for n, a in G.items():
        assert np.all(np.isfinite(a)), (grid, state, k, n)
    if state == "noise" and k >= -300:
        for n, a in G.items():
            assert np.any(a != 0.0), (grid, k, n)
    if state == "plateau":
        # constant blocks: exact zeros where every flux difference vanishes, and enough cells beside a step that the rung says something
        zero = np.mean([np.mean(tendencies[grid].g_cpu.interior_cells(G[n]) == 0.0) for n in ("c0", "c1")])
        print(f"grid {grid} plateau({k}): {100 * zero:.1f} % of the tracer tendencies are exactly 0")
        assert zero >= 0.05, (grid, k, zero)
        assert 1.0 - zero >= 0.50, (grid, k, zero)


@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_the_split_of_the_ladders_at_the_float32_reciprocal_limit(tendencies, grid):
    """IN_DOMAIN is exactly the set of rungs on which no smoothness indicator + eps reaches 2^126, the documented limit of the kernels' fast
    Float32 reciprocal: a criterion on the state, computed here in numpy, not on what the kernels return"""
    for state, k in V.LADDER:
        tendencies[grid](V.state_of(V.GRIDS[grid], state, k))
        top = V.largest_indicator(tendencies[grid].parents()) + 1e-8
        print(f"grid {grid} {state}({k}): largest beta + eps = 2^{np.log2(top):.1f}")
        assert (top < V.FLOAT32_RECIPROCAL_LIMIT) == ((state, k) in V.IN_DOMAIN), (grid, state, k, top)
    assert sorted(V.OBSERVED_DEVIATION) == sorted((g, s, k) for g in V.GRIDS for s, k in V.OUT_OF_DOMAIN)


def test_the_noise_ladder_crosses_both_float32_limits():
    """max over the tracers of the curvature term every smoothness indicator contains: below 2^126 (a normal Float32 reciprocal) up to
    rung 55, above 2^128 (Float32 overflow) from rung 66 on"""
    for name, grid in V.GRIDS.items():
        for k in V.NOISE_RUNGS:
            vals = V.noise(grid, k)
            top = max(float(V.curvature_indicator_bound_x(vals[n]).max()) for n in ("c0", "c1"))
            print(f"grid {name} noise({k}): max 13/12 (d2 c)^2 = 2^{np.log2(top) if top > 0 else -np.inf:.1f}")
            if k >= 66:
                assert top >= 2.0 ** 128, (name, k, top)
            if k <= 55:
                assert top < 2.0 ** 126, (name, k, top)


def test_the_oracles_newton_div_is_ieee_beyond_float32(oracle):
    L = oracle.lib()
    a = 1.7 * 2.0 ** 120
    assert L.oro_newton_div_f32(a, 2.0 ** 128) == 0.0 and np.signbit(L.oro_newton_div_f32(a, 2.0 ** 128)) == False      # noqa: E712
    assert L.oro_newton_div_f32(a, 1e300) == 0.0
    for b in (2.0 ** 126, 2.0 ** 127, FLT_MAX, 1.37 * 2.0 ** 126, 1.9 * 2.0 ** 127):
        inv = np.float64(np.float32(1.0) / np.float32(b))                  # a subnormal Float32 above 2^126: kept, not flushed
        assert inv > 0.0
        x = np.float64(a) * inv
        # fma(fma(x, -b, a), inv, x) in exact rational arithmetic, rounded once per fma
        from fractions import Fraction as Fr
        inner = float(Fr(float(x)) * Fr(-b) + Fr(a))
        want = float(Fr(inner) * Fr(float(inv)) + Fr(float(x)))
        assert L.oro_newton_div_f32(a, b) == want, (b, L.oro_newton_div_f32(a, b), want)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_one_non_finite_cell_has_a_small_footprint(tendencies, grid, value):
    g = V.GRIDS[grid]
    cells = int(np.prod(g.size))
    for field, cell in V.NONFINITE_CELLS[grid]:
        G = tendencies[grid](V.nonfinite_at(g, field, cell, value))
        counts = {n: int(np.sum(~np.isfinite(a))) for n, a in G.items()}
        print(f"grid {grid} {value} in {field} at {cell}: non-finite tendencies {counts} of {cells} cells")
        for n, c in counts.items():
            assert c <= 0.02 * cells, (grid, field, n, c)
            if n in V.REACH[field]:
                assert c >= 1, (grid, field, n)
                if np.isnan(value):
                    assert int(np.sum(np.isnan(G[n]))) == c, (grid, field, n)
            else:
                assert c == 0, (grid, field, n)


@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_the_selection_cases_have_a_cell_only_selection_keeps_clean(tendencies, grid):
    """in each case of SELECTION_CASES the reference's Gc0 is finite at `clean`, NaN at the NaN's own cell, and every other tendency is
    untouched: the clean cell is what a kernel that blends instead of selecting, or selects the other side at a tie, turns into NaN"""
    g = V.GRIDS[grid]
    H = 3
    for name, cell, pins, clean in V.SELECTION_CASES[grid]:
        G = tendencies[grid](V.selection_state(g, cell, pins))
        at = lambda c: tuple(q + H for q in c)            # noqa: E731
        assert np.isfinite(G["c0"][at(clean)]), (grid, name)
        assert np.isnan(G["c0"][at(cell)]), (grid, name)
        # the NaN sits three cells (tie) or one cell (wall) from the clean one along x: both x faces of the clean cell are in play
        assert abs((cell[0] - clean[0] + g.size[0] // 2) % g.size[0] - g.size[0] // 2) in (1, 3) and cell[1:] == clean[1:], (grid, name)
        for n in ("u", "v", "w", "c1"):
            assert np.all(np.isfinite(G[n])), (grid, name, n)
        print(f"grid {grid} {name}: Gc0 NaN in {int(np.isnan(G['c0']).sum())} cells, finite at {clean}")


@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_the_patch_at_rest_has_ties_of_both_signs_and_no_negative_zero(tendencies, grid):
    g = V.GRIDS[grid]
    vals = V.rest_patch(g)
    blk = V.REST_BLOCK[grid]
    for n in V.FACE_DIRECTION:
        assert np.all(vals[n][blk] == 0.0) and vals[n][blk].shape == (10, 4, 3)
    for n in ("c0", "c1"):
        assert np.any(vals[n][blk] > 0) and np.any(vals[n][blk] < 0)
    G = tendencies[grid](vals)
    for n, a in G.items():
        assert np.all(np.isfinite(a)), n
        assert not np.any(np.signbit(a) & (a == 0.0)), (grid, n)


def test_largest_weight_sum_of_the_ladders():
    """the largest argument the Float64 reciprocal of the weight normalisation meets on the two ladders (x direction, numpy restatement):
    finite, and printed for the comparison with the reciprocal's measured limit in the GPU test"""
    top = V.largest_weight_sum()
    print(f"largest sum(alpha) over both ladders and grids: 2^{np.log2(top):.1f}")
    assert np.isfinite(top) and top > 1e51            # past what exponents 0 .. 160 sample
