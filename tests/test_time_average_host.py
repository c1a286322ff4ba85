"""CPU tests of the time averages (oldoceananigans_jl_amd/time_averages.py, units.py, the Simulation's diagnostics): the schedule's truth
table at its boundaries, the strings and units of the reference (OutputWriters/windowed_time_average.jl:49-57,75-98; Utils/prettytime.jl;
Units.jl), and the bookkeeping of advance_time_average! (:232-262) driven by a stub clock -- the product's time_fold against the
independent restatement tests/time_average_reference.py AND against triples worked out by hand from the reference lines. Nothing
touches a device: grids have architecture None, fields are borrowed."""
import ctypes as C
import types
import warnings

import pytest

import oldoceananigans_jl_amd as ocn
import time_average_reference as TA
from oldoceananigans_jl_amd import time_averages, units

CCC = (ocn.Center, ocn.Center, ocn.Center)


def stub_model(time=0.0, iteration=0):
    return types.SimpleNamespace(clock=types.SimpleNamespace(time=float(time), iteration=iteration))


def stub_average(schedule):
    """what time_fold needs of a WindowedTimeAverage"""
    return types.SimpleNamespace(schedule=schedule, window_start_time=0.0, window_start_iteration=0, previous_collection_time=0.0, _first=False)


def drive(schedule, times):
    """the Simulation's order with a stub clock: at iteration 0 the diagnostic is run unconditionally (run.jl:232-235), afterwards where
    its schedule says so (:153-154). Returns [(time, iteration, (T_previous, Δt, T_current, first) or None)] and the stub average"""
    avg, model, out = stub_average(schedule), stub_model(), []
    for iteration, time in enumerate(times):
        model.clock.time, model.clock.iteration = float(time), iteration
        fold = time_averages.time_fold(avg, model.clock) if (iteration == 0 or schedule(model)) else None
        out.append((float(time), iteration, fold))
    return out, avg


# ---------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------
def test_schedule_truth_table_at_the_boundaries():
    s = ocn.AveragedTimeInterval(4, window=2.5)
    assert (s.interval, s.window, s.stride, s.first_actuation_time, s.actuations, s.collecting) == (4.0, 2.5, 1, 0.0, 0, False)
    assert s.next_actuation_time() == 4.0
    below, at_start, inside, at_end = (stub_model(t, 1) for t in (1.0, 1.5, 1.5000000000000002, 4.0))
    # time == next - window: not scheduled (strict >, :90) and outside the window (<=, :94)
    assert not s(at_start) and s.outside_window(at_start.clock)
    assert not s(below) and s.outside_window(below.clock)
    assert s(inside) and not s.outside_window(inside.clock) and not s.end_of_window(inside.clock)
    # time == next: the end of the window (>=, :95)
    assert s(at_end) and s.end_of_window(at_end.clock) and not s.end_of_window(stub_model(3.9999999999999996).clock)
    s.collecting = True
    assert s(below)                                            # collecting || ...
    s.collecting, s.actuations = False, 1
    assert s.next_actuation_time() == 8.0 and not s(at_end) and s(stub_model(5.6))
    # aligned_time_step: the fallback, Δt unchanged (Utils/schedules.jl:15)
    assert s.aligned_time_step(at_start.clock, 10.0) == 10.0
    c = s.copy()
    assert (c.interval, c.window, c.stride, c.actuations, c.collecting) == (4.0, 2.5, 1, 0, False) and c is not s
    t = s.TimeInterval()
    assert isinstance(t, ocn.TimeInterval) and t.interval == 4.0
    assert ocn.AveragedTimeInterval(3).window == 3.0 and ocn.AveragedTimeInterval(3, stride=2).stride == 2
    assert s.initialize(at_start) is False and s.first_actuation_time == 0.0


def test_window_longer_than_the_interval_is_an_error():
    with pytest.raises(ValueError, match=r"Averaging window 5 is greater than the output interval 4\."):
        ocn.AveragedTimeInterval(4, window=5)


def test_repr_is_the_jldoctest():
    s = ocn.AveragedTimeInterval(4 * units.days, window=2 * units.days)
    assert repr(s) == s.summary() == "AveragedTimeInterval(window=2 days, stride=1, interval=4 days)"
    assert repr(ocn.AveragedTimeInterval(10 * units.minutes, window=90, stride=3)) == "AveragedTimeInterval(window=1.500 minutes, stride=3, interval=10 minutes)"


def test_prettytime_known_answers():
    """every branch of prettytime / prettytimeunits (prettytime.jl:20-64), worked out from those lines"""
    for t, long, short in ((0, "0 seconds", "0 s"), (1e-10, "1.000e-10 seconds", "1.000e-10 s"), (2e-7, "200 ns", "200 ns"), (0.002, "2 ms", "2 ms"),
                           (0.0125, "12.500 ms", "12.500 ms"), (1, "1 second", "1 s"), (30.5, "30.500 seconds", "30.500 s"), (59, "59 seconds", "59 s"),
                           (60, "1 minute", "1 m"), (90, "1.500 minutes", "1.500 m"), (3600, "1 hour", "1 hr"), (7200.0, "2 hours", "2 hrs"),
                           (86400, "1 day", "1 d"), (2 * 86400.0, "2 days", "2 d"), (129600, "1.500 days", "1.500 d")):
        assert ocn.prettytime(t) == long and ocn.prettytime(t, False) == short, t
    assert ocn.prettytime(2.5e-5).endswith(" μs")


def test_units():
    assert ocn.units is units
    assert (units.second, units.minute, units.hour, units.day) == (1.0, 60.0, 3600.0, 86400.0)
    assert (units.seconds, units.minutes, units.hours, units.days) == (1.0, 60.0, 3600.0, 86400.0)
    assert all(isinstance(getattr(units, n), float) for n in ("second", "seconds", "minute", "minutes", "hour", "hours", "day", "days"))
    assert not hasattr(units, "meter") and not hasattr(units, "KiB")


# ---------------------------------------------------------------------------------------------------------------------
# advance_time_average!: the triples
# ---------------------------------------------------------------------------------------------------------------------
HAND = {
    # (window, stride): {time: (T_previous, Δt, T_current)} for AveragedTimeInterval(4, ...), Δt = 1, t = 0..4
    (2.0, 1): {3.0: (0.0, 1.0, 1.0), 4.0: (1.0, 1.0, 2.0)},
    (2.5, 1): {2.0: (0.0, 0.5, 0.5), 3.0: (0.5, 1.0, 1.5), 4.0: (1.5, 1.0, 2.5)},
    (2.5, 2): {3.0: (0.0, 1.5, 1.5), 4.0: (1.5, 1.0, 2.5)},
    (4.0, 1): {1.0: (0.0, 1.0, 1.0), 2.0: (1.0, 1.0, 2.0), 3.0: (2.0, 1.0, 3.0), 4.0: (3.0, 1.0, 4.0)},
}


@pytest.mark.parametrize("window,stride", sorted(HAND))
def test_triples_equal_the_hand_worked_cases_and_the_restatement(window, stride):
    got, avg = drive(ocn.AveragedTimeInterval(4, window=window, stride=stride), range(5))
    want = HAND[(window, stride)]
    assert {t: f[:3] for t, _, f in got if f is not None} == want
    # the first sample of the window, and only that one, is marked
    firsts = [f[3] for _, _, f in got if f is not None]
    assert firsts == [True] + [False] * (len(want) - 1)
    ref, ref_schedule = TA.triples(4, window, stride, [(float(t), t) for t in range(5)])
    assert [(t, i, None if f is None else f[:3]) for t, i, f in got] == ref
    s = avg.schedule
    assert s.actuations == ref_schedule.actuations == 1 and s.collecting is ref_schedule.collecting is False
    assert avg.window_start_time == 4.0 - window and avg.previous_collection_time == 4.0


def test_a_full_window_starts_at_iteration_one_never_zero():
    got, avg = drive(ocn.AveragedTimeInterval(4, window=4), [0.0])
    assert got == [(0.0, 0, None)] and avg.schedule.collecting is False and avg.window_start_iteration == 0
    got, avg = drive(ocn.AveragedTimeInterval(4, window=4), [0.0, 1.0])
    assert got[1][2] == (0.0, 1.0, 1.0, True) and avg.schedule.collecting is True
    assert avg.window_start_iteration == 0 and avg.window_start_time == 0.0
    # even a clock that is past the window's start at iteration 0 collects nothing there (:234)
    avg, model = stub_average(ocn.AveragedTimeInterval(4, window=4)), stub_model(2.0, 0)
    assert time_averages.time_fold(avg, model.clock) is None and avg.schedule.collecting is False


@pytest.mark.parametrize("stride", [1, 2])
def test_a_second_window_starts_afresh(stride):
    got, avg = drive(ocn.AveragedTimeInterval(4, window=2.5, stride=stride), range(9))
    folds = {t: f for t, _, f in got if f is not None}
    first = HAND[(2.5, stride)]
    assert {t: f[:3] for t, f in folds.items() if t <= 4} == first
    # the same triples four time units later, the first of them marked as the first of its window again
    assert {t - 4: f[:3] for t, f in folds.items() if t > 4} == first
    assert [f[3] for t, f in sorted(folds.items()) if t > 4] == [True] + [False] * (len(first) - 1)
    assert avg.schedule.actuations == 2 and avg.schedule.collecting is False and avg.window_start_time == 5.5
    ref, ref_schedule = TA.triples(4, 2.5, stride, [(float(t), t) for t in range(9)])
    assert [(t, i, None if f is None else f[:3]) for t, i, f in got] == ref and ref_schedule.actuations == 2


def test_unequal_steps_and_a_window_that_ends_between_steps():
    """steps that do not land on the window's end: the window closes at the first time >= next_actuation_time (:95)"""
    times = [0.0, 0.7, 1.9, 2.6, 3.1, 4.3, 5.0, 6.2, 7.9, 8.4]
    for stride in (1, 2, 3):
        got, avg = drive(ocn.AveragedTimeInterval(4, window=2.5, stride=stride), times)
        ref, ref_schedule = TA.triples(4, 2.5, stride, [(t, i) for i, t in enumerate(times)])
        assert [(t, i, None if f is None else f[:3]) for t, i, f in got] == ref, stride
        assert avg.schedule.actuations == ref_schedule.actuations == 2
    assert got[5][2][:3] == (3.1 - 1.5, 4.3 - 3.1, 4.3 - 1.5)


def test_restatement_fold_is_the_reference_statement():
    import numpy as np
    r, s = np.array([0.0, 1.5, -2.0]), np.array([-0.0, 3.0, 0.1])
    first = TA.fold(np.zeros(3), s, 0.0, 0.5, 0.5)
    assert TA.same_bits(first, (0.0 * 0.0 + s * 0.5) / 0.5) and not np.signbit(first[0])      # -0.0 gives +0.0
    assert TA.same_bits(TA.fold(r, s, 0.5, 1.0, 1.5), (r * 0.5 + s * 1.0) / 1.5)
    assert not TA.same_bits(np.array([0.0]), np.array([-0.0]))
    assert TA.same_bits(TA.fold_samples([s, r], [(0.0, 0.5, 0.5), (0.5, 1.0, 1.5)]), (first * 0.5 + r * 1.0) / 1.5)


# ---------------------------------------------------------------------------------------------------------------------
# refusals, before the library is initialised
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device():
    schedule = ocn.AveragedTimeInterval(4, window=2)
    grid = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1))
    T = ocn.Field(CCC, grid, data=C.c_void_p(0))
    with pytest.raises(NotImplementedError, match="callable"):
        ocn.WindowedTimeAverage(lambda model: 1.0, schedule=schedule)
    with pytest.raises(NotImplementedError, match="fetch_operand"):
        ocn.WindowedTimeAverage(T, schedule=schedule, fetch_operand=False)
    with pytest.raises(TypeError):
        ocn.WindowedTimeAverage("T", schedule=schedule)
    with pytest.raises(TypeError, match="AveragedTimeInterval"):
        ocn.WindowedTimeAverage(T, schedule=ocn.TimeInterval(4))
    part = ocn.RectilinearGrid(None, size=(8, 8, 8), extent=(1, 1, 1), topology=(ocn.FullyConnected, ocn.Periodic, ocn.Bounded))
    P = ocn.Field(CCC, part, data=C.c_void_p(0))
    with pytest.raises(NotImplementedError, match="partitioned"):
        ocn.WindowedTimeAverage(P, schedule=schedule)
    # Callback(wta, schedule) (callback.jl:90-92); Callback(wta) takes the average's schedule (:81-88)
    wta = ocn.WindowedTimeAverage.__new__(ocn.WindowedTimeAverage)
    wta.schedule = schedule
    with pytest.raises(ValueError, match="Schedule must be inferred from WindowedTimeAverage"):
        ocn.Callback(wta, ocn.IterationInterval(1))
    assert ocn.Callback(wta).schedule is schedule


def test_simulation_has_diagnostics_and_the_names_are_exported():
    for name in ("WindowedTimeAverage", "AveragedTimeInterval", "advance_time_average", "run_diagnostic", "prettytime", "units", "time_averages"):
        assert name in ocn.__all__, name
    model = types.SimpleNamespace(velocities=types.SimpleNamespace(u=None), clock=stub_model().clock)
    sim = ocn.Simulation(model, Δt=1.0, stop_time=4.0)
    assert isinstance(sim.diagnostics, dict) and not sim.diagnostics and list(sim.callbacks)[0] == "stop_time_exceeded"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wta = ocn.WindowedTimeAverage.__new__(ocn.WindowedTimeAverage)
        wta.schedule, wta.model, wta.result = ocn.AveragedTimeInterval(4, window=2), None, "the result"
        assert wta(stub_model(1.0, 1)) == "the result"          # not collecting, stride 1: no warning
    wta.schedule.collecting = True
    with pytest.warns(UserWarning, match="before the collection period is complete"):
        wta(stub_model(3.0, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wta(stub_model(0.0, 0))                                 # iteration 0: no warning (:202-204)
    wta.schedule = ocn.AveragedTimeInterval(4, window=2, stride=2)
    with pytest.warns(UserWarning, match="stride > 1"):
        wta(stub_model(1.0, 1))
