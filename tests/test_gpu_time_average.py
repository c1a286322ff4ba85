"""GPU tests of the time averages: the fold at the store of every diagnostics kernel (csrc/ocn_diagnostics.h: dg_store; include/
ocn_mi355x.h: ocn_time_average_*) and WindowedTimeAverage / AveragedTimeInterval / Simulation.diagnostics on top of it, against
tests/time_average_reference.py (the schedule, advance_time_average! and the fold as separate numpy operations).

What is compared how:
  * computed fields, accumulations, maxima and minima have a defined operation order: the sample comes from tests/diagnostics_reference.py
    or tests/stencil_reference.py and the folded result must have the BITS of the numpy fold (compared as int64: the sign of zero counts);
  * sums and averages: the samples are what the plain entry points (ocn_reduce_*) write into a separate Field(scan) -- they give the
    same bits on every call -- and the result must have the bits of the numpy fold of those; it must ALSO lie within a derived bound of
    the exact value: with S_s = math.fsum of sample s's terms and b_s its summation bound (n 2⁻⁵³ Σ|xᵢ| for a sum, (2n + 2) 2⁻⁵³ Σ|xᵢ| / V
    for an average, tests/test_gpu_diagnostics.py), the weighted mean Σ_s S_s Δt_s / T (exact, in rationals) is met within
    max_s b_s + 4 N 2⁻⁵³ max_s |S_s| for N samples: the weights sum to one, and a fold step makes four roundings, each at most 2⁻⁵³ of a
    value no larger than the largest sample.
The first sample of every window is folded into a result that holds NaN: the first-sample mode must not read it.

Grids: those of tests/test_gpu_diagnostics.py -- rows longer than a wave and no multiple of 64, more rows per output than one chunk
(the combine kernel), a stretched z, a Flat direction."""
import ctypes as C
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

import diagnostics_reference as D
import stencil_reference as R
import time_average_reference as TA
from helpers import smooth_state
from test_gpu_stencil_diagnostics import Case

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GRIDS = ("bpb_stretched", "slice", "ppp")
# AveragedTimeInterval(4, window=2.5) with Δt = 1 (tests/test_time_average_host.py) and one more step: unequal weights
TIMES = ((0.0, 0.5, 0.5), (0.5, 1.0, 1.5), (1.5, 1.0, 2.5), (2.5, 1.0, 3.5))
REDUCED_DIMS = ((1,), (1, 2, 3), (2,), (2, 3))        # x reduced in one chunk; x reduced, combined chunks; x kept (twice)


@pytest.fixture(scope="module")
def cases(ocn, oracle, arch):
    return {n: Case(ocn, oracle, arch, n) for n in GRIDS}


def fresh_parents(c, seed):
    """new seeded values everywhere, halos included"""
    rng = np.random.default_rng(seed)
    for n in "Tuvw":
        a = np.asfortranarray(0.5 + rng.standard_normal(c.f[n].shape))
        c.f[n].set_parent(a)
        c.p[n] = a


def nan_result(ocn, loc, grid):
    f = ocn.Field(loc, grid)
    f.set_parent(np.full(f.shape, np.nan))
    return f


def mask_of(dims):
    return sum(1 << (d - 1) for d in dims)


def reduced(loc, dims):
    return tuple(None if d + 1 in dims else l for d, l in enumerate(loc))


def row_sums(terms, metric, count, axes, average):
    """per output element: (exact S or S / V as a Fraction, its summation bound)"""
    kept = [d for d in range(3) if d not in axes]
    rows = lambda a: np.transpose(a, kept + list(axes)).reshape(int(np.prod([a.shape[d] for d in kept])), -1)     # noqa: E731
    x = rows(terms)
    m = rows(metric) if metric is not None else None
    n, out = x.shape[1], []
    for q in range(x.shape[0]):
        S, A = math.fsum(x[q].tolist()), math.fsum(np.abs(x[q]).tolist())
        if average:
            V = math.fsum(m[q].tolist()) if m is not None else float(count)
            out.append((Fraction(S) / Fraction(V), (2 * n + 2) * U * A / V))
        else:
            out.append((Fraction(S), n * U * A))
    return out


def assert_fold_within_bound(got, stats, times, axes, tag):
    """got: the reduced interior; stats: row_sums of every sample (over `axes`). The bound of the module docstring, the worst ratio
    returned"""
    g = np.transpose(got, [d for d in range(3) if d not in axes] + list(axes)).reshape(-1)
    T = Fraction(times[-1][2])
    worst = 0.0
    assert g.size == len(stats[0]), tag
    for q in range(g.size):
        want = sum(s[q][0] * Fraction(t[1]) for s, t in zip(stats, times)) / T
        bound = max(s[q][1] for s in stats) + 4 * len(times) * U * max(abs(float(s[q][0])) for s in stats)
        err = abs(Fraction(float(g[q])) - want)
        worst = max(worst, float(err) / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, (tag, q, g[q], float(want), float(err), bound)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the fold arithmetic of every kernel, both evaluators
# ---------------------------------------------------------------------------------------------------------------------
class Folded:
    """one operand of one kernel: the launch that folds it, what the sample should be, and the numpy fold of the samples so far"""

    def __init__(self, tag, result, launch, sample, exact, stats=None):
        self.tag, self.result, self.launch, self.sample, self.exact, self.stats = tag, result, launch, sample, exact, stats
        self.samples, self.all_stats = [], []


def build(ocn, c):
    """the Folded of every kernel family for the fixed evaluator (w * u, and T as the plain inner operand of a scan) and the interpreter
    (two recorded programs)"""
    K, grid = ocn.kernels, c.grid
    T, u, w = c.f["T"], c.f["u"], c.f["w"]
    by_field = lambda: {c.f[n]: c.p[n] for n in "Tuvw"}                                                  # noqa: E731
    out = []
    fixed = [("w*u", w * u), ("T", T)]
    programs = [(n, ocn.KernelFunctionOperation(R.KERNEL_FUNCTIONS[n][0], R.KERNEL_FUNCTIONS[n][1], grid, *[c.f[a] for a in R.KERNEL_FUNCTIONS[n][2]]))
                for n in ("vorticity", "w_dzT_ccc")]

    def fixed_value(op):
        return lambda dims_mask=0, absolute=False: D.evaluate(grid, D.operand_of(op, by_field()), dims_mask, absolute)

    def program_value(name, k):
        def value(dims_mask=0, absolute=False):
            v = R.SLICES[name](grid, *[c.p[a] for a in R.KERNEL_FUNCTIONS[name][2]])
            v = np.abs(v) if absolute else v
            if not dims_mask:
                return v, None
            m = D.metric(grid, k.location, dims_mask)
            return v * m, np.broadcast_to(m, v.shape)
        return value

    for stencil, table in ((False, fixed), (True, programs)):
        for name, op in table:
            loc = tuple(op.location if hasattr(op, "location") else op.loc)
            value = program_value(name, op) if stencil else fixed_value(op)
            ev = "stencil" if stencil else "fixed"
            # computed field (the plain field T has its own test below: the whole parent)
            if name != "T":
                res = nan_result(ocn, loc, grid)
                fold = K.time_average_stencil if stencil else K.time_average_operation
                out.append(Folded((ev, name, "compute"), res, lambda t, fold=fold, op=op, res=res: fold(grid, op, t, res),
                                  lambda value=value: value()[0], True))
            # accumulations: along x (rows kernel), y and z (cols kernel), forward and reverse, with and without the metric
            for dim, reverse, metric in ((1, False, True), (2, True, False), (3, False, True), (3, True, False)):
                res = nan_result(ocn, loc, grid)
                fold = K.time_average_accumulate_stencil if stencil else K.time_average_accumulate_operation

                def sample(value=value, dim=dim, reverse=reverse, metric=metric):
                    v = value(1 << (dim - 1) if metric else 0)[0]
                    return np.flip(np.cumsum(np.flip(v, axis=dim - 1), axis=dim - 1), axis=dim - 1) if reverse else np.cumsum(v, axis=dim - 1)
                out.append(Folded((ev, name, "accumulate", dim, reverse, metric), res,
                                  lambda t, fold=fold, op=op, res=res, dim=dim, reverse=reverse, metric=metric: fold(grid, op, dim, reverse, metric, t, res),
                                  sample, True))
            for dims in REDUCED_DIMS:
                rloc, mask, axes = reduced(loc, dims), mask_of(dims), tuple(d - 1 for d in dims)
                fold = K.time_average_reduce_stencil if stencil else K.time_average_reduce_operation
                plain = K.reduce_stencil if stencil else K.reduce_operation
                # extrema: a defined order
                for kind, absolute in (("maximum", False), ("minimum", True)):
                    res = nan_result(ocn, rloc, grid)
                    red = np.max if kind == "maximum" else np.min
                    out.append(Folded((ev, name, kind, dims, absolute), res,
                                      lambda t, fold=fold, op=op, res=res, kind=kind, dims=dims, absolute=absolute: fold(grid, op, kind, dims, False, absolute, t, res),
                                      lambda value=value, red=red, axes=axes, absolute=absolute: red(value(0, absolute)[0], axis=axes, keepdims=True), True))
                # sums and averages: the sample is what the plain entry point writes
                stretched = 3 in dims and not grid.z_regular
                for kind, metric in (("sum", False), ("sum", True), ("average", stretched)):
                    res, separate = nan_result(ocn, rloc, grid), ocn.Field(rloc, grid)

                    def sample(plain=plain, op=op, kind=kind, dims=dims, metric=metric, separate=separate):
                        plain(grid, op, kind, dims, metric, False, separate)
                        return separate.interior()

                    def stats(value=value, mask=mask, metric=metric, kind=kind, axes=axes):
                        terms, m = value(mask if metric else 0)
                        count = int(np.prod([terms.shape[d] for d in axes]))
                        return row_sums(terms, m if (metric and kind == "average") else None, count, axes, kind == "average")
                    out.append(Folded((ev, name, kind, dims, metric, axes), res,
                                      lambda t, fold=fold, op=op, res=res, kind=kind, dims=dims, metric=metric: fold(grid, op, kind, dims, metric, False, t, res),
                                      sample, False, stats))
    return out


@pytest.mark.parametrize("name", GRIDS)
def test_fold_arithmetic_of_every_kernel(ocn, cases, name):
    c = cases[name]
    folded = build(ocn, c)
    assert len(folded) == 4 * (4 + 4 * 5) + 3              # per operand: 4 accumulations, 4 dims x (2 extrema + 3 sums); 3 computed fields
    for s, (Tp, dt, Tc) in enumerate(TIMES):
        fresh_parents(c, 1000 + s)
        for f in folded:
            f.samples.append(np.array(f.sample()))
            if f.stats is not None:
                f.all_stats.append(f.stats())
            f.launch((Tp, dt, Tc, s == 0))
        for f in folded:
            got = f.result.interior()
            want = TA.fold_samples(f.samples, TIMES[:s + 1])
            assert not np.isnan(got).any(), (name, f.tag, s)
            assert TA.same_bits(got, want), (name, f.tag, s, np.argwhere(got != want)[:4])
    worst = 0.0
    for f in folded:
        if f.stats is not None:
            worst = max(worst, assert_fold_within_bound(f.result.interior(), f.all_stats, TIMES, f.tag[-1], (name, f.tag)))
        # only the interior is written: the halos of the result still hold what they held
        p = f.result.parent()
        p[f.result._interior_slices()] = np.nan
        assert np.isnan(p).all(), (name, f.tag)
    print(f"{name}: largest error / bound of the folded sums = {worst:.3f}")


@pytest.mark.parametrize("name", GRIDS)
def test_first_sample_of_negative_zero_is_positive_zero(ocn, cases, name):
    """(0.0 * 0.0 + (-0.0) * Δt) / T_current = +0.0 (windowed_time_average.jl:224 after :238), from a result that holds NaN"""
    c = cases[name]
    K, grid = ocn.kernels, c.grid
    CCC = (ocn.Center,) * 3
    Z = ocn.Field(CCC, grid)
    Z.set_parent(np.full(Z.shape, -0.0))
    assert np.signbit(Z.parent()).all()
    first = (0.0, 0.5, 0.5, True)
    fixed, program = Z * 1.0, ocn.KernelFunctionOperation(CCC, lambda i, j, k, grid, z: z[i, j, k] * 1.0, grid, Z)
    # the operand IS -0.0 everywhere: what the plain entry points write
    for op, compute in ((fixed, K.compute_operation), (program, K.compute_stencil)):
        plain = ocn.Field(CCC, grid)
        compute(grid, op, plain)
        assert np.signbit(plain.interior()).all() and not plain.interior().any()
    launches = []
    for op, st in ((fixed, False), (program, True)):
        launches.append((CCC, lambda r, op=op, st=st: (K.time_average_stencil if st else K.time_average_operation)(grid, op, first, r)))
        for dim in (1, 2, 3):
            launches.append((CCC, lambda r, op=op, st=st, dim=dim: (K.time_average_accumulate_stencil if st else K.time_average_accumulate_operation)(
                grid, op, dim, False, False, first, r)))
        for dims in REDUCED_DIMS:
            for kind in ("sum", "maximum", "minimum"):
                launches.append((reduced(CCC, dims), lambda r, op=op, st=st, dims=dims, kind=kind: (K.time_average_reduce_stencil if st else K.time_average_reduce_operation)(
                    grid, op, kind, dims, False, False, first, r)))
    launches.append((CCC, lambda r: K.time_average_operation(grid, Z, first, r)))                   # the plain field: the whole parent
    for q, (loc, launch) in enumerate(launches):
        r = nan_result(ocn, loc, grid)
        launch(r)
        got = r.parent() if q == len(launches) - 1 else r.interior()
        assert TA.same_bits(got, np.zeros(got.shape)), (name, q)
    # ... and a later sample of -0.0 keeps what the reference keeps: (r * Tp + (-0.0) * Δt) / Tc with r = +0.0 is +0.0
    r = nan_result(ocn, CCC, grid)
    K.time_average_operation(grid, fixed, first, r)
    K.time_average_operation(grid, fixed, (0.5, 1.0, 1.5, False), r)
    assert TA.same_bits(r.interior(), np.zeros(r.interior().shape))


@pytest.mark.parametrize("name", GRIDS)
def test_plain_field_is_folded_over_the_whole_parent(ocn, cases, name):
    c = cases[name]
    for n in "Tuw":
        f = c.f[n]
        r = nan_result(ocn, f.loc, c.grid)
        samples = []
        for s, (Tp, dt, Tc) in enumerate(TIMES):
            fresh_parents(c, 2000 + s)
            samples.append(c.p[n].copy())
            ocn.kernels.time_average_operation(c.grid, f, (Tp, dt, Tc, s == 0), r)
            assert TA.same_bits(r.parent(), TA.fold_samples(samples, TIMES[:s + 1])), (name, n, s)


# ---------------------------------------------------------------------------------------------------------------------
# WindowedTimeAverage with a model
# ---------------------------------------------------------------------------------------------------------------------
MODELS = {"ppp_16": ((16, 16, 16), ("Periodic",) * 3, (0.0, 1.0)), "bbb_12x10x8": ((12, 10, 8), ("Bounded",) * 3, (-1.0, 0.0))}
DT = 1.0 / 128            # a dyadic step below the 0.1 Δx / 0.6 of tests/golden: 4 DT, 2.5 DT and the window's edges are exact


def make_model(ocn, arch, name, zero=False):
    size, topo, z = MODELS[name]
    grid = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=tuple(getattr(ocn, t) for t in topo))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=("T", "S"))
    if zero:
        ocn.set_model(model, u=0, v=0, w=0, T=0, S=0)
    else:
        ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, seed=1234))
    return model


def test_reference_instantiate_windowed_time_average(ocn, arch):
    """run_instantiate_windowed_time_average_tests (test/test_output_writers.jl:15-28)"""
    model = make_model(ocn, arch, "ppp_16")
    u = model.velocities.u
    u0 = u.parent()
    assert u0.any()
    wta = ocn.WindowedTimeAverage(u, schedule=ocn.AveragedTimeInterval(10, window=1))
    assert wta.result is not u and wta.result.loc == u.loc
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(wta(model).parent(), u0)
    # an operation and a scan start as their current values too (:180-183)
    f = model.fields()
    w, T = f["w"], f["T"]
    parents = {x: x.parent() for x in f.values()}
    wT = ocn.WindowedTimeAverage(w * T, model, schedule=ocn.AveragedTimeInterval(10, window=1))
    assert wT.location == (ocn.Center, ocn.Center, ocn.Face) and wT.result.operand is None
    assert np.array_equal(wT.result.interior(), D.compute_operation(model.grid, D.operand_of(w * T, parents)))
    avg = ocn.WindowedTimeAverage(ocn.Average(T, dims=(1, 2)), model, schedule=ocn.AveragedTimeInterval(10, window=1))
    assert avg.location == (None, None, ocn.Center) and avg.result.interior().shape == (1, 1, 16)
    assert np.array_equal(avg.result.interior(), ocn.Field(ocn.Average(T, dims=(1, 2))).interior())


def test_reference_time_step_with_windowed_time_average(ocn, arch):
    """time_step_with_windowed_time_average (test/test_output_writers.jl:30-44)"""
    model = make_model(ocn, arch, "ppp_16", zero=True)
    wta = ocn.WindowedTimeAverage(model.velocities.u, schedule=ocn.AveragedTimeInterval(4, window=2))
    simulation = ocn.Simulation(model, Δt=1.0, stop_time=4.0)
    simulation.diagnostics["u_avg"] = wta
    ocn.run(simulation)
    assert model.clock.time == 4.0 and model.clock.iteration == 4
    assert wta.schedule.actuations == 1 and wta.schedule.collecting is False
    assert np.array_equal(wta(model).parent(), model.velocities.u.parent())


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_a_real_run_equals_the_restatement(ocn, arch, name, stride):
    """two windows of AveragedTimeInterval(4, window=2.5) (in units of the step) through Simulation.diagnostics: the model's parents are
    copied after every step, the restatements evaluated on them and folded with the triples of time_average_reference.py"""
    model = make_model(ocn, arch, name)
    grid, f = model.grid, model.fields()
    u, v, w, T = f["u"], f["v"], f["w"], f["T"]
    FFC = (ocn.Face, ocn.Face, ocn.Center)
    schedule = ocn.AveragedTimeInterval(4 * DT, window=2.5 * DT, stride=stride)
    operands = {"u": u, "wT": w * T, "Tbar": ocn.Average(T, dims=(1, 2)), "zeta": ocn.KernelFunctionOperation(FFC, ocn.operators.ζ3ᶠᶠᶜ, grid, u, v),
                "wT_field": ocn.Field(w * T), "Tbar_field": ocn.Field(ocn.Average(T, dims=(1, 2)))}
    wtas = {n: ocn.WindowedTimeAverage(op, model, schedule=schedule.copy()) for n, op in operands.items()}
    simulation = ocn.Simulation(model, Δt=DT, stop_time=8 * DT)
    for n, wta in wtas.items():
        simulation.diagnostics[n] = wta
    assert list(simulation.diagnostics) == list(operands)
    separate = ocn.Field(ocn.Average(T, dims=(1, 2)), compute=False)
    state = {}

    def integrand(n):
        P = state["parents"]
        if n == "u":
            return P[u]
        if n == "wT":
            return D.compute_operation(grid, D.operand_of(operands["wT"], P))
        if n == "zeta":
            return R.vorticity(grid, P[u], P[v])
        return ocn.compute(separate).interior()

    refs = {n: TA.Average(TA.Schedule(4 * DT, 2.5 * DT, stride), np.zeros(wtas[n].result.shape if n == "u" else wtas[n].result.interior().shape))
            for n in ("u", "wT", "Tbar", "zeta")}
    stats, times, checked = [], [], 0
    for step in range(1, 9):
        simulation.time_step()
        time, iteration = model.clock.time, model.clock.iteration
        # the RK3 clock adds three stage increments: a time may miss step * DT by an ulp -- the restatement is given the clock's own times
        assert iteration == step and abs(time - step * DT) <= 4 * np.spacing(step * DT)
        state["parents"] = {x: x.parent() for x in f.values()}
        for n, ref in refs.items():
            triple = ref.advance(time, iteration, lambda n=n: integrand(n)) if ref.schedule.scheduled(time) else None
            if triple is None:
                continue
            checked += 1
            got = wtas[n].result.parent() if n == "u" else wtas[n].result.interior()
            assert TA.same_bits(got, ref.result), (name, stride, n, step, triple)
            if n == "Tbar" and step > 4:                       # the second window: the terms of its samples, for the bound
                terms, _, count = D.reduce_terms(grid, D.operand_of(T, state["parents"]), 3, False)
                stats.append(row_sums(terms, None, count, (0, 1), True))
                times.append(triple)
        # in flight equals materialised: the computed fields are computed first (fetch_output), then folded over their whole parents
        assert TA.same_bits(wtas["wT"].result.interior(), wtas["wT_field"].result.interior()), (name, stride, step)
        assert TA.same_bits(wtas["Tbar"].result.interior(), wtas["Tbar_field"].result.interior()), (name, stride, step)
    assert checked == 4 * 2 * (3 if stride == 1 else 2)
    assert model.clock.time == 8 * DT
    for n, wta in wtas.items():
        assert wta.schedule.actuations == 2 and wta.schedule.collecting is False, n
        assert wta.window_start_time == 5.5 * DT and wta.previous_collection_time == 8 * DT
    for n, ref in refs.items():
        assert ref.schedule.actuations == 2 and not ref.schedule.collecting
    worst = assert_fold_within_bound(wtas["Tbar"].result.interior(), stats, times, (0, 1), (name, stride, "Tbar"))
    print(f"{name}, stride {stride}: largest error / bound of the averaged profile = {worst:.3f}")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        wtas["u"](model)
    assert len(caught) == (1 if stride > 1 else 0)


def test_callback_of_a_windowed_time_average(ocn, arch):
    """Callback(wta) (Simulations/callback.jl:81-88) advances the average on its own schedule, as the diagnostic does"""
    model = make_model(ocn, arch, "ppp_16")
    w, T = model.fields()["w"], model.fields()["T"]
    a = ocn.WindowedTimeAverage(w * T, model, schedule=ocn.AveragedTimeInterval(4 * DT, window=2.5 * DT))
    b = ocn.WindowedTimeAverage(w * T, model, schedule=ocn.AveragedTimeInterval(4 * DT, window=2.5 * DT))
    simulation = ocn.Simulation(model, Δt=DT, stop_time=4 * DT)
    simulation.diagnostics["a"] = a
    simulation.callbacks["b"] = ocn.Callback(b)
    start = a.result.interior()
    ocn.run(simulation)
    assert a.schedule.actuations == b.schedule.actuations == 1
    assert TA.same_bits(a.result.interior(), b.result.interior()) and not np.array_equal(a.result.interior(), start)


# ---------------------------------------------------------------------------------------------------------------------
# the raw C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_refuse_bad_folds_before_any_launch(ocn, arch, cases):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    EINVAL, ENOTSUP = -1, -2
    c = cases["ppp"]
    T, u = c.f["T"], c.f["u"]
    result = ocn.Field(T.loc, c.grid)
    pattern = np.asfortranarray(np.random.default_rng(5).standard_normal(result.shape))
    result.set_parent(pattern)
    good = ocn.diagnostics.operand_struct(T * u)
    plain = ocn.diagnostics.operand_struct(T)
    st, keep = ocn.kernels._stencil_struct(ocn.dz(T) * 1.0)
    fold = lambda *t: C.byref(_lib.TimeFold(*t))                                                         # noqa: E731
    ok = fold(0.5, 1.0, 1.5, 0)

    def calls(operand, stencil, f, out):
        g = c.grid.handle
        if stencil:
            return (lambda: L.ocn_time_average_stencil(g, operand, f, out), lambda: L.ocn_time_average_reduce_stencil(g, operand, 0, 3, 0, 0, f, out),
                    lambda: L.ocn_time_average_accumulate_stencil(g, operand, 2, 0, 0, f, out))
        return (lambda: L.ocn_time_average_operation(g, operand, f, out), lambda: L.ocn_time_average_reduce_operation(g, operand, 0, 3, 0, 0, f, out),
                lambda: L.ocn_time_average_accumulate_operation(g, operand, 2, 0, 0, f, out))

    inf, nan = math.inf, math.nan
    bad_folds = [((nan, 1.0, 1.5, 0), b"finite"), ((0.5, inf, 1.5, 0), b"finite"), ((0.5, 1.0, inf, 0), b"finite"), ((-inf, 1.0, 1.5, 0), b"finite"),
                 ((0.0, 1.0, 0.0, 0), b"T_current"), ((0.5, 1.0, -1.5, 0), b"T_current"), ((-0.5, 1.0, 1.5, 0), b"T_previous"),
                 ((0.5, 1.0, 1.5, 1), b"first sample")]
    for operand, stencil in ((C.byref(good), False), (C.byref(plain), False), (C.byref(st), True)):
        for t, word in bad_folds:
            for call in calls(operand, stencil, fold(*t), result.data):
                assert call() == EINVAL and word in L.ocn_last_error(), (t, L.ocn_last_error())
        for call in calls(operand, stencil, None, result.data) + calls(operand, stencil, ok, None) + calls(None, stencil, ok, result.data):
            assert call() == EINVAL and b"NULL" in L.ocn_last_error()
    # the fold of a whole parent array of any shape
    n = result.nbytes // 8
    for t, word in bad_folds:
        assert L.ocn_time_average_parent(T.data, n, fold(*t), result.data) == EINVAL and word in L.ocn_last_error()
    for call in (lambda: L.ocn_time_average_parent(None, n, ok, result.data), lambda: L.ocn_time_average_parent(T.data, n, None, result.data),
                 lambda: L.ocn_time_average_parent(T.data, n, ok, None)):
        assert call() == EINVAL and b"NULL" in L.ocn_last_error()
    assert L.ocn_time_average_parent(T.data, 0, ok, result.data) == EINVAL
    # every operand error of the plain entry points
    g = c.grid.handle
    assert L.ocn_time_average_reduce_operation(g, C.byref(good), 0, 0, 0, 0, ok, result.data) == EINVAL and b"dims_mask" in L.ocn_last_error()
    assert L.ocn_time_average_reduce_operation(g, C.byref(good), 4, 1, 0, 0, ok, result.data) == EINVAL
    assert L.ocn_time_average_reduce_operation(g, C.byref(good), 1, 1, 1, 0, ok, result.data) == EINVAL           # maximum takes no metric
    assert L.ocn_time_average_accumulate_operation(g, C.byref(good), 3, 0, 0, ok, result.data) == EINVAL
    assert L.ocn_time_average_reduce_stencil(g, C.byref(st), 0, 8, 0, 0, ok, result.data) == EINVAL and b"dims_mask" in L.ocn_last_error()
    assert L.ocn_time_average_accumulate_stencil(g, C.byref(st), -1, 0, 0, ok, result.data) == EINVAL
    bad = ocn.diagnostics.operand_struct(T * u)
    bad.loc[:] = [1, 0, 0]
    assert L.ocn_time_average_operation(g, C.byref(bad), ok, result.data) == EINVAL and b"location" in L.ocn_last_error()
    bad = ocn.diagnostics.operand_struct(T)
    bad.op = 9
    assert L.ocn_time_average_operation(g, C.byref(bad), ok, result.data) == EINVAL
    ocn.synchronize()
    assert TA.same_bits(result.parent(), pattern)                      # nothing was launched: the result keeps its bits
    # a connected (partitioned) grid handle is refused by the library itself
    part = ocn.RectilinearGrid(arch, size=(16, 16, 16), x=(0.0, 1.0), y=(0.0, 1.0), z=(0.0, 1.0), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    pc, pout = ocn.Field(T.loc, part), ocn.Field(T.loc, part)
    operand = _lib.Operand()
    operand.op, operand.a = 0, pc.data
    for call in (lambda: L.ocn_time_average_operation(part.handle, C.byref(operand), ok, pout.data),
                 lambda: L.ocn_time_average_reduce_operation(part.handle, C.byref(operand), 0, 3, 0, 0, ok, pout.data),
                 lambda: L.ocn_time_average_accumulate_operation(part.handle, C.byref(operand), 2, 0, 0, ok, pout.data)):
        assert call() == ENOTSUP and b"partitioned" in L.ocn_last_error()
    pst = _lib.StencilOperand()
    program, pst.n = ocn.operators.program_array([(ocn.operators.OPS["load"], 0, 0, 0, 0, 0, 0, 0.0)])
    ptrs, locs = (C.c_void_p * 1)(pc.data), (C.c_int * 3)(0, 0, 0)
    pst.program, pst.args, pst.arg_locs, pst.nargs = program, ptrs, locs, 1
    assert L.ocn_time_average_stencil(part.handle, C.byref(pst), ok, pout.data) == ENOTSUP and b"partitioned" in L.ocn_last_error()
    ocn.synchronize()
    assert not pout.parent().any()
