"""Time-averaged diagnostics (reference: src/OutputWriters/windowed_time_average.jl, all of it except AveragedSpecifiedTimes;
src/Utils/prettytime.jl; src/Simulations/run.jl:150-163,212-245 and callback.jl:81-92 are in simulations.py).

    wT = ocn.WindowedTimeAverage(w * T, model, schedule=ocn.AveragedTimeInterval(10 * minutes, window=2 * minutes))
    simulation.diagnostics["wT"] = wT                    # advanced after every time-step
    wT(model).interior()                                 # the mean over the last complete window

The operand is a Field (plain or computed), an operation or a scan. Operations and scans are evaluated IN FLIGHT: the diagnostics kernel
forms the value and folds it into `result` at its store (ocn_time_average_*, csrc/ocn_diagnostics.h: dg_store), no array in between.
The halos of such a result are not defined; `result.interior()` is the product. A Field is folded over its whole parent array, halos
included, as the reference's broadcast over parent(result) does.

The bookkeeping -- which iterations collect, and the (T_previous, Δt, T_current) of each -- is time_fold below: it reads a clock (anything
with `time` and `iteration`) and touches no device. One deviation from windowed_time_average.jl:238: the result is not zeroed when a
window opens. The first sample of the window is folded in the library's "first sample" mode, which gives the bits of the zeroed result
without reading it; with stride > 1 the result therefore keeps the previous window's mean between the opening of a window and its first
on-stride sample, where the reference holds zeros (wta(model) warns in both while the window collects).

Refused (NotImplementedError, before anything touches the device): a callable operand, fetch_operand=False, a partitioned grid.
Not built: AveragedSpecifiedTimes, output writers, checkpointing a window in progress."""
import math
import warnings

from . import units
from .fields import Field


def _maybe_int(t):
    """maybe_int (prettytime.jl:6)"""
    return int(t) if float(t).is_integer() else t


def prettytime(t, longform=True):
    """prettytime(t, longform=true) (Utils/prettytime.jl:20-36): seconds as a string in ns .. days with three decimal places, whole
    values without any"""
    s = "seconds" if longform else "s"
    if t == 0:
        return f"0 {s}"
    if t < 1e-9:
        return f"{t:.3e} {s}"
    value, name = _prettytimeunits(_maybe_int(t), longform)
    return f"{int(value):d} {name}" if float(value).is_integer() else f"{value:.3f} {name}"


def _prettytimeunits(t, longform):
    """prettytimeunits (prettytime.jl:38-64)"""
    if t < 1e-6:
        return t * 1e9, "ns"
    if t < 1e-3:
        return t * 1e6, "μs"
    if t < 1:
        return t * 1e3, "ms"
    if t < units.minute:
        return t, ("s" if not longform else ("second" if t == 1 else "seconds"))
    if t < units.hour:
        value = _maybe_int(t / units.minute)
        return value, ("m" if not longform else ("minute" if value == 1 else "minutes"))
    if t < units.day:
        value = _maybe_int(t / units.hour)
        return value, (("hour" if longform else "hr") if value == 1 else ("hours" if longform else "hrs"))
    value = _maybe_int(t / units.day)
    return value, ("d" if not longform else ("day" if value == 1 else "days"))


class AveragedTimeInterval:
    """AveragedTimeInterval(interval; window=interval, stride=1) (windowed_time_average.jl:15-22,75-98): averages over the `window` that
    ends at every multiple of `interval`, a sample every `stride` iterations inside it"""

    def __init__(self, interval, window=None, stride=1):
        window = interval if window is None else window
        if window > interval:
            raise ValueError(f"Averaging window {window} is greater than the output interval {interval}.")
        self.interval, self.window, self.stride = float(interval), float(window), int(stride)
        self.first_actuation_time, self.actuations, self.collecting = 0.0, 0, False

    def next_actuation_time(self):
        """the end of the averaging window (:80-86)"""
        return self.first_actuation_time + (self.actuations + 1) * self.interval

    def __call__(self, model):
        return self.collecting or model.clock.time > self.next_actuation_time() - self.window      # strict (:89-92)

    def initialize(self, model):
        """initialize_schedule!(sch::AveragedTimeInterval, clock) = nothing (:93)"""
        return False

    def outside_window(self, clock):
        return clock.time <= self.next_actuation_time() - self.window

    def end_of_window(self, clock):
        return clock.time >= self.next_actuation_time()

    def aligned_time_step(self, clock, Δt):
        """no schedule_aligned_time_step method: the fallback (Utils/schedules.jl:15)"""
        return Δt

    def copy(self):
        return AveragedTimeInterval(self.interval, window=self.window, stride=self.stride)

    def TimeInterval(self):
        """TimeInterval(sch::AveragedTimeInterval) (:97)"""
        from .simulations import TimeInterval
        return TimeInterval(self.interval)

    def summary(self):
        """Base.summary (:269-272)"""
        return f"AveragedTimeInterval(window={prettytime(self.window)}, stride={self.stride}, interval={prettytime(self.interval)})"

    __repr__ = summary


def _operand_kind(operand):
    """"field" | "operation" | "scan"; the refusals that need no device"""
    from . import diagnostics
    if isinstance(operand, Field):
        return "field"
    if isinstance(operand, diagnostics._NODES):
        return "operation"
    if isinstance(operand, diagnostics.Scan):
        return "scan"
    if callable(operand):
        raise NotImplementedError("a callable operand (a function that returns an array or a number) is not built: a WindowedTimeAverage takes "
                                  "a Field, an operation or a scan")
    raise TypeError(f"WindowedTimeAverage({type(operand).__name__}): a Field, an operation (BinaryOperation, Derivative, UnaryOperation, "
                    "KernelFunctionOperation) or a scan")


class WindowedTimeAverage:
    """WindowedTimeAverage(operand, model=nothing; schedule, fetch_operand=true) (windowed_time_average.jl:151-190): the running average of
    `operand` over schedule.window, recurring every schedule.interval; `result` starts as the operand's current value"""

    def __init__(self, operand, model=None, schedule=None, fetch_operand=True):
        from . import diagnostics
        kind = _operand_kind(operand)
        if not fetch_operand:
            raise NotImplementedError("fetch_operand=False (an operand that is folded as the array it is) is not built")
        if not isinstance(schedule, AveragedTimeInterval):
            raise TypeError("schedule: an AveragedTimeInterval (AveragedSpecifiedTimes is not built)")
        diagnostics._check_grid(operand.grid)
        self.operand, self.model, self.schedule, self.fetch_operand = operand, model, schedule, True
        self.window_start_time, self.window_start_iteration, self.previous_collection_time = 0.0, 0, 0.0
        self._first = False                                   # the window is open and has no sample yet
        # result = similar(output); result .= output (:180-183)
        if kind == "field":
            from . import _lib
            diagnostics.compute_at(operand, None if model is None else model.clock.time)         # fetch_output (fetch_output.jl:14-17)
            self.result = Field(operand.loc, operand.grid)
            _lib.check(_lib.lib().ocn_memcpy_d2d(self.result.data, operand.data, operand.nbytes))
        else:
            self.result = Field(operand)
            self.result.operand = self.result.status = None  # a plain field from here on: what compute() did once the fold does later

    # location(wta) = location(wta.operand) (:193)
    @property
    def location(self):
        return self.result.loc

    def parent(self):
        return self.result.parent()

    def __call__(self, model=None):
        """(wta::WindowedTimeAverage)(model) (:199-209)"""
        model = self.model if model is None else model
        if self.schedule.collecting and model is not None and model.clock.iteration > 0:
            warnings.warn("Returning a WindowedTimeAverage before the collection period is complete.")
        if self.schedule.stride > 1:
            warnings.warn("WindowedTimeAverage can be erroneous when stride > 1 and either the timestep is variable or there are floating point "
                          "rounding errors in times, both of which result in a decoupling of the model clock times (used in the OutputWriters) "
                          "and iteration numbers (used for stride).")
        return self.result


def time_fold(wta, clock):
    """advance_time_average! (windowed_time_average.jl:232-262) without the arithmetic: updates the window's bookkeeping for the clock's
    time and iteration and returns (T_previous, Δt, T_current, first) when this iteration adds a sample -- accumulate_result!'s three
    times (:218-221) and whether it is the first of its window -- else None. No device is involved: `wta` needs `schedule`,
    `window_start_time`, `window_start_iteration`, `previous_collection_time` and `_first`."""
    sch = wta.schedule
    time, iteration = clock.time, clock.iteration
    if iteration == 0 or sch.outside_window(clock):
        return None
    if not sch.collecting:
        # (the reference zeroes the result here, :238: the first sample's fold mode stands for it)
        sch.collecting = True
        wta._first = True
        wta.window_start_time = sch.next_actuation_time() - sch.window
        wta.previous_collection_time = wta.window_start_time
        wta.window_start_iteration = iteration - 1
    end = sch.end_of_window(clock)
    if not end and (iteration - wta.window_start_iteration) % sch.stride != 0:
        return None                                           # off stride
    fold = (wta.previous_collection_time - wta.window_start_time, time - wta.previous_collection_time, time - wta.window_start_time, wta._first)
    wta.previous_collection_time = time
    wta._first = False
    if end:
        sch.collecting = False
        sch.actuations += 1
    return fold


def accumulate_result(wta, fold):
    """accumulate_result! (:216-230) for the times of time_fold: one launch (two where a reduction has more chunks than one block adds),
    no copy to the host, no synchronisation"""
    from . import diagnostics, kernels
    T_previous, Δt, T_current, first = fold
    if not (math.isfinite(T_previous) and math.isfinite(Δt) and math.isfinite(T_current)):
        raise ValueError(f"the clock gives no finite averaging times: {fold[:3]}")
    operand, result, grid = wta.operand, wta.result, wta.result.grid
    times = (T_previous, Δt, T_current, first)
    if isinstance(operand, Field):
        model = wta.model
        diagnostics.compute_at(operand, None if model is None else model.clock.time)
        if any(l is None for l in operand.loc):
            kernels.time_average_parent(operand, times, result)          # a reduced (computed) field
        else:
            kernels.time_average_operation(grid, operand, times, result)
        return
    inner = operand.operand if isinstance(operand, diagnostics.Scan) else operand
    stencil = not (isinstance(inner, Field) or (isinstance(inner, diagnostics.BinaryOperation) and inner.fixed))      # as diagnostics.compute
    if not isinstance(operand, diagnostics.Scan):
        (kernels.time_average_stencil if stencil else kernels.time_average_operation)(grid, operand, times, result)
    elif operand.reducing:
        (kernels.time_average_reduce_stencil if stencil else kernels.time_average_reduce_operation)(
            grid, inner, operand.kind, operand.dims, operand.use_metric, operand.absolute, times, result)
    else:
        (kernels.time_average_accumulate_stencil if stencil else kernels.time_average_accumulate_operation)(
            grid, inner, operand.dims[0], operand.reverse, operand.use_metric, times, result)


def advance_time_average(wta, model):
    """advance_time_average!(wta, model) (:232-262)"""
    fold = time_fold(wta, model.clock)
    if fold is not None:
        if wta.model is None:
            wta.model = model
        accumulate_result(wta, fold)


def run_diagnostic(diagnostic, model):
    """run_diagnostic!(wta::WindowedTimeAverage, model) = advance_time_average!(wta, model) (:265)"""
    if isinstance(diagnostic, WindowedTimeAverage):
        return advance_time_average(diagnostic, model)
    return diagnostic.run_diagnostic(model)
