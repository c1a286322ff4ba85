"""numpy restatement of the time averages (reference: OutputWriters/windowed_time_average.jl:15-22,75-98,216-262), independent of the
package's time_averages.py: the schedule, advance_time_average! as a function of (time, iteration) that returns the three times of
accumulate_result!, and the fold as separate numpy operations (elementwise IEEE doubles, no fused multiply-add). The restatement zeroes
the result when a window opens, as the reference does (:238), and always reads it: the product's "first sample" mode has to give
these bits without doing either."""
import numpy as np


class Schedule:
    """AveragedTimeInterval (:15-22,75-98)"""

    def __init__(self, interval, window=None, stride=1):
        self.interval = float(interval)
        self.window = self.interval if window is None else float(window)
        self.stride = stride
        self.first_actuation_time, self.actuations, self.collecting = 0.0, 0, False

    def next_actuation_time(self):
        return self.first_actuation_time + (self.actuations + 1) * self.interval

    def scheduled(self, time):
        return self.collecting or time > self.next_actuation_time() - self.window

    def outside_window(self, time):
        return time <= self.next_actuation_time() - self.window

    def end_of_window(self, time):
        return time >= self.next_actuation_time()


class Average:
    """the bookkeeping of a WindowedTimeAverage (:151-159) and, when `result` is an array, its arithmetic"""

    def __init__(self, schedule, result=None):
        self.schedule, self.result = schedule, result
        self.window_start_time, self.window_start_iteration, self.previous_collection_time = 0.0, 0, 0.0

    def advance(self, time, iteration, integrand=None):
        """advance_time_average! (:232-262): returns (T_previous, Δt, T_current) when a sample is added, else None. integrand: a host
        array, or a function that returns one (called only when a sample is added)"""
        s = self.schedule
        if iteration == 0 or s.outside_window(time):
            return None
        if not s.collecting:
            if self.result is not None:
                self.result[...] = 0
            s.collecting = True
            self.window_start_time = s.next_actuation_time() - s.window
            self.previous_collection_time = self.window_start_time
            self.window_start_iteration = iteration - 1
        if s.end_of_window(time):
            times = self._accumulate(time, integrand)
            s.collecting = False
            s.actuations += 1
            return times
        if (iteration - self.window_start_iteration) % s.stride == 0:
            return self._accumulate(time, integrand)
        return None

    def _accumulate(self, time, integrand):
        """accumulate_result! (:216-230)"""
        dt = time - self.previous_collection_time
        T_current = time - self.window_start_time
        T_previous = self.previous_collection_time - self.window_start_time
        if self.result is not None:
            sample = integrand() if callable(integrand) else integrand
            self.result[...] = fold(self.result, sample, T_previous, dt, T_current)
        self.previous_collection_time = time
        return (T_previous, dt, T_current)


def fold(result, integrand, T_previous, dt, T_current):
    """result = (result * T_previous + integrand * Δt) / T_current (:224): two multiplies, an add, a divide"""
    a = np.multiply(result, np.float64(T_previous))
    b = np.multiply(integrand, np.float64(dt))
    return np.divide(np.add(a, b), np.float64(T_current))


def fold_samples(samples, times):
    """the running average of `samples` (arrays of one shape) taken with the `times` triples, the first into a zeroed result"""
    result = np.zeros_like(np.asarray(samples[0], dtype=np.float64))
    for sample, (T_previous, dt, T_current) in zip(samples, times):
        result = fold(result, sample, T_previous, dt, T_current)
    return result


def triples(interval, window, stride, clock):
    """[(time, iteration, triple or None) for every (time, iteration) of `clock`] and the schedule afterwards; the average is advanced
    only where the schedule says so (Simulations/run.jl:153-154), iteration 0 as at initialize! (:232-235)"""
    schedule = Schedule(interval, window, stride)
    avg = Average(schedule)
    out = []
    for time, iteration in clock:
        t = avg.advance(time, iteration) if (iteration == 0 or schedule.scheduled(time)) else None
        out.append((time, iteration, t))
    return out, schedule


def same_bits(a, b):
    """== with the sign of zero: the arrays compared as int64"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
