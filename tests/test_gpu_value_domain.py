"""The tendency kernels outside the O(1) binades of the other parity tests: the states of value_domain_cases.py (powers-of-two ladders of
noise and of plateau-and-step fields, one NaN or +Inf on a tile seam or beside a wall, a patch of fluid exactly at rest) against the
oracle, compared as BIT PATTERNS on the whole parent array -- so -0.0 is not +0.0 -- with NaNs compared by position. The oracle is plain C
with IEEE divides; tests/test_value_domain_host.py certifies that it is finite and non-trivial on every state used here. The fast
reciprocals are swept over their whole exponent range through the debug hooks, and the pressure solve's linear passes are checked for
homogeneity under powers of two.

Durations measured on the MI355X: DESIGN.md 3.2."""
import ctypes as C

import numpy as np
import pytest

import value_domain_cases as V
from poisson_cases import SOLVER_CASES, case_id, white_noise_interiors, z_faces_of, z_of
import poisson_reference as PR

pytestmark = pytest.mark.gpu

PATH_KEYS = ("split_solve_active", "fused_zfft_active", "c2r_strided_active")


class _Pair:
    """the GPU model and the oracle model of one grid, reused by every case on that grid"""

    def __init__(self, ocn, oracle, arch, grid):
        self.ocn, self.grid = ocn, grid
        g = ocn.RectilinearGrid(arch, size=grid.size, x=(0.0, 1.0), y=(0.0, 1.0), z=V.z_of(grid),
                                topology=tuple(getattr(ocn, t) for t in grid.topology))
        self.model = ocn.NonhydrostaticModel(grid=g, advection=ocn.WENO(), tracers=V.GPU_NAMES[3:3 + grid.ntracers])
        self.oracle = V.OracleTendencies(oracle, grid)

    def tendencies(self, vals):
        """{impl: {field: parent array}} on the GPU, {field: parent array} of the oracle"""
        ocn, m = self.ocn, self.model
        want = self.oracle(vals)
        ocn.set_model(m, enforce_incompressibility=False, **{g: vals[n] for g, n in zip(V.GPU_NAMES, V.FIELDS)})
        got = {}
        try:
            for impl in self.grid.impls:
                m.set_option("tendency_impl", impl)
                for g in V.GPU_NAMES:
                    m.tendency(g).set_parent(np.zeros(m.tendency(g).shape))
                ocn.update_state(m, True)
                got[impl] = {n: np.array(m.tendency(g).parent()) for g, n in zip(V.GPU_NAMES, V.FIELDS)}
        finally:
            m.set_option("tendency_impl", 2)
        return got, want


@pytest.fixture(scope="module")
def pairs(ocn, oracle, arch):
    made = {name: _Pair(ocn, oracle, arch, grid) for name, grid in V.GRIDS.items()}
    yield made
    for p in made.values():
        p.model.close()


def _differing(a, b):
    """number of cells whose bit patterns differ (NaN against NaN counts as equal)"""
    na, nb = np.isnan(a), np.isnan(b)
    ua, ub = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return int(np.sum((na != nb) | (~na & ~nb & (ua != ub))))


@pytest.mark.parametrize("state,k", V.IN_DOMAIN, ids=lambda p: str(p))
@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_scaled_states_match_the_oracle_bit_for_bit(pairs, grid, state, k, record_property):
    """every rung on which all smoothness indicators + eps stay below 2^126, the domain of the kernels' Float32 reciprocal (the host test
    checks that split on the states themselves): noise 2^-600 .. 2^55, plateaus 2^0 .. 2^60"""
    got, want = pairs[grid].tendencies(V.state_of(V.GRIDS[grid], state, k))
    report = {(impl, n): (_differing(G[n], want[n]), int(np.sum(~np.isfinite(G[n])))) for impl, G in got.items() for n in V.FIELDS}
    bad = {key: v for key, v in report.items() if v != (0, 0)}
    print(f"grid {grid} {state}({k}): (impl, field) -> (cells that differ from the oracle, non-finite cells): {bad or 'none'}")
    record_property("cells_differing", sum(v[0] for v in report.values()))
    for impl, G in got.items():
        for n in V.FIELDS:
            assert np.all(np.isfinite(want[n])), (n, "the oracle is not finite: the host test certifies this rung")
            assert np.array_equal(np.isfinite(G[n]), np.isfinite(want[n])), (grid, state, k, impl, n, report[impl, n])
            assert V.same_bits(G[n], want[n]), (grid, state, k, impl, n, report[impl, n])


@pytest.mark.parametrize("state,k", V.OUT_OF_DOMAIN, ids=lambda p: str(p))
@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_known_deviation_beyond_the_float32_reciprocal_range(pairs, grid, state, k):
    """PINS A KNOWN DEVIATION FROM THE REFERENCE, it does not state a requirement. On these rungs (noise from 2^60, plateaus from 2^63) some
    beta + eps reaches 2^126. The oracle, with IEEE divides, stays finite on all of them (host test); rcp_rn_f32<1> returns 0 where the
    reciprocal is subnormal and NaN where Float32(beta + eps) is +inf (ocn_device.h), so the kernels' tendencies differ from the oracle's
    and from 2^61 on are mostly NaN. A range test in front of the reciprocal restores bit parity on every rung (measured with it: all 52
    ladder cases equal the oracle) but costs 0.9 - 1.7 % of the 256^3 step, so the deviation stands. Pinned here: the number of cells that
    differ and of non-finite cells as measured, and that the three implementations deviate IDENTICALLY. If this test fails because the
    counts went to (0, 0), the range has been extended: move the rung to IN_DOMAIN."""
    got, want = pairs[grid].tendencies(V.state_of(V.GRIDS[grid], state, k))
    assert all(np.all(np.isfinite(a)) for a in want.values())
    first = got[V.GRIDS[grid].impls[0]]
    for impl, G in got.items():
        observed = (sum(_differing(G[n], want[n]) for n in V.FIELDS), sum(int(np.sum(~np.isfinite(G[n]))) for n in V.FIELDS))
        print(f"grid {grid} {state}({k}) impl {impl}: (cells that differ from the oracle, non-finite cells) = {observed}")
        assert observed == V.OBSERVED_DEVIATION[grid, state, k], (grid, state, k, impl, observed)
        for n in V.FIELDS:
            assert V.same_bits(G[n], first[n]), (grid, state, k, impl, n)


@pytest.mark.parametrize("case", [(g, f, c) for g in sorted(V.GRIDS) for f, c in V.NONFINITE_CELLS[g]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_a_nan_spreads_exactly_as_in_the_oracle(pairs, case):
    grid, field, cell = case
    for value in (np.nan, np.inf):
        got, want = pairs[grid].tendencies(V.nonfinite_at(V.GRIDS[grid], field, cell, value))
        assert sum(int(np.isnan(a).sum()) for a in want.values()) >= 1
        for impl, G in got.items():
            for n in V.FIELDS:
                where = (grid, field, cell, value, impl, n)
                assert np.array_equal(np.isnan(G[n]), np.isnan(want[n])), (where, np.argwhere(np.isnan(G[n]) != np.isnan(want[n]))[:8])
                assert V.same_bits(G[n], want[n]), (where, _differing(G[n], want[n]))


@pytest.mark.parametrize("case", [(g,) + c for g in sorted(V.GRIDS) for c in V.SELECTION_CASES[g]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_an_unselected_nan_stays_out(pairs, case):
    """the upwind SELECTION itself (value_domain_cases.SELECTION_CASES): a NaN on the side the reference does not select, at a face whose
    advecting velocity is exactly 0 and at the UpwindBiased{1} faces beside a wall. With finite data a kernel that selects the other side at
    the tie, or blends the two sides with weights 0 and 1, returns the reference's bits (the flux is multiplied by 0, the kernels end in
    -div + 0.0); here it writes a NaN into a cell the oracle keeps finite (the host test checks that it does)."""
    grid, name, cell, pins, clean = case
    got, want = pairs[grid].tendencies(V.selection_state(V.GRIDS[grid], cell, pins))
    assert np.isfinite(want["c0"][tuple(q + 3 for q in clean)])
    for impl, G in got.items():
        for n in V.FIELDS:
            where = (grid, name, impl, n)
            assert np.array_equal(np.isnan(G[n]), np.isnan(want[n])), (where, np.argwhere(np.isnan(G[n]) != np.isnan(want[n]))[:8])
            assert V.same_bits(G[n], want[n]), (where, _differing(G[n], want[n]))


@pytest.mark.parametrize("grid", sorted(V.GRIDS))
def test_zero_velocity_patch_and_signed_zeros(pairs, grid):
    """fluid exactly at rest in a block: the oracle's bits including the sign of every zero. This pins the signed zeros and the tie with
    finite data; it cannot see WHICH side a tie selects (a flux times 0 is +-0 either way) -- test_an_unselected_nan_stays_out does."""
    got, want = pairs[grid].tendencies(V.rest_patch(V.GRIDS[grid]))
    for impl, G in got.items():
        for n in V.FIELDS:
            assert np.array_equal(np.signbit(G[n]), np.signbit(want[n])), (grid, impl, n)
            assert V.same_bits(G[n], want[n]), (grid, impl, n, _differing(G[n], want[n]))
            assert not np.any(np.signbit(G[n]) & (G[n] == 0.0)), (grid, impl, n)             # the kernels end in -div + 0.0


RCP64_WINDOWS = ((160, 300), (300, 600), (600, 900), (900, 1020), (-1020, -60))


def test_fast_reciprocals_over_their_whole_domain(record_property):
    """rcp_rn_f32<1> exhaustively on every binade from 2^64 up to the last one whose reciprocal is a normal Float32 (2^125: 1 / x > 2^-126);
    on 2^126 and 2^127, where the IEEE reciprocal is subnormal, the count is recorded (measured: 8388607 and 8388608 of 2^23 -- v_rcp_f32
    flushes the subnormal result; only 1 / 2^126 = 2^-126 itself agrees). rcp_rn_f64 on 2^24 samples per exponent window up to 2^1020 and down to 2^-1020: the first window with a mismatch is its limit,
    and that limit has to lie 20 binades above the largest sum(alpha) the ladders of value_domain_cases.py produce."""
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    bad = C.c_ulonglong()
    counts = {}
    for e in range(64, 128):
        _lib.check(L.ocn_debug_rcp_check(1, e, C.byref(bad)))
        counts[e] = bad.value
    print("rcp_rn_f32<1> mismatches per binade 64 .. 127:", {e: c for e, c in counts.items() if c} or "none")
    record_property("rcp32_mismatches_2^126", counts[126])
    record_property("rcp32_mismatches_2^127", counts[127])
    for e in range(64, 126):
        assert counts[e] == 0, (e, counts[e])
    limit = None
    for lo, hi in RCP64_WINDOWS:
        _lib.check(L.ocn_debug_rcp64_check(1 << 24, lo, hi, 4242 + hi, C.byref(bad)))
        print(f"rcp_rn_f64 mismatches on exponents [{lo}, {hi}]: {bad.value} of 2^24")
        if bad.value and limit is None and lo > 0:
            limit = lo
        if lo < 0:
            assert bad.value == 0, (lo, hi, bad.value)              # 1 / sum(alpha) never goes there (sum >= 1): exact all the same
    top = np.log2(V.largest_weight_sum())
    limit_text = "none up to 2^1020" if limit is None else f"2^{limit}"
    print(f"largest sum(alpha) of the ladders 2^{top:.1f}; first window of rcp_rn_f64 with a mismatch: {limit_text}")
    record_property("rcp64_first_bad_exponent", -1 if limit is None else limit)
    assert (1020 if limit is None else limit) >= top + 20, (limit, top)


HOMOGENEITY_CASES = {c.path: c for c in SOLVER_CASES if (c.path, c.size) in {
    ("split-tridiagonal", (126, 8, 10)), ("split-fused-z", (126, 8, 8)), ("plain-tridiagonal", (12, 6, 10)), ("flat", (66, 1, 16))}
    or (c.path, c.topology, c.kind) == ("cosine", ("Bounded",) * 3, 1) and c.size == (11, 13, 9)}


@pytest.mark.parametrize("path", sorted(HOMOGENEITY_CASES))
def test_linear_steps_are_homogeneous(ocn, arch, path):
    """divergence, transforms, tridiagonal solve and correction are linear, and scaling by a power of two is exact in every one of their
    operations: pNHS of 2^k x white noise is 2^k x pNHS of the noise, bit for bit, unless a pass takes a data-dependent shortcut.

    Each scaling is solved by a model of its own. The tridiagonal solve is NOT a function of its right-hand side alone: like the reference's
    (batched_tridiagonal_solver.jl:234-237), the sweep leaves the last level of the singular (kx, ky) = (0, 0) column at whatever the
    solution buffer held, i.e. at the previous solve's value. That shifts the column by a constant which the mean removal takes out again
    -- up to the rounding of `constant + solution`. Measured with ONE model for the three solves: split-tridiagonal 2814 and
    plain-tridiagonal 1322 cells of pNHS differ in their last bits at 2^40; the other three paths are homogeneous either way. A new
    solver's buffer is zero, so here every solve starts from the same state and any difference left is a property of the passes.
    Repeated solves on one model are NOT covered by this test."""
    case = HOMOGENEITY_CASES[path]
    geom = PR.Geometry(case.size, case.topology, z_faces_of(case))
    vals = white_noise_interiors(geom, _NoTracers(case))
    p = {}
    for k in (0, 40, -300):
        grid = ocn.RectilinearGrid(arch, size=case.size, x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(case), topology=tuple(getattr(ocn, t) for t in case.topology))
        model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=())
        try:
            paths = tuple(model.get_option(key) for key in PATH_KEYS)
            assert paths == case.paths, (paths, case.paths)
            ocn.set_model(model, enforce_incompressibility=True, **{n: np.ldexp(vals[n], k) for n in "uvw"})
            p[k] = np.array(model.pressures.pNHS.parent())
        finally:
            model.close()
    print(case_id(case), dict(zip(PATH_KEYS, case.paths)))
    assert np.all(np.isfinite(p[0])) and np.any(p[0] != 0.0)
    for k in (40, -300):
        assert V.same_bits(p[k], np.ldexp(p[0], k)), (case_id(case), k, _differing(p[k], np.ldexp(p[0], k)))


class _NoTracers:
    """a solver case as white_noise_interiors reads it: the case's seed, no tracers"""
    ntracers = 0

    def __init__(self, case):
        self._case = case

    def __getattr__(self, name):
        return getattr(self._case, name)
