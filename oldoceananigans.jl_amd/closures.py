"""Turbulence closures on the accelerated path: ScalarDiffusivity with constant isotropic ν, κ and explicit or
vertically implicit time discretisation (reference: TurbulenceClosures/turbulence_closure_implementations/scalar_diffusivity.jl), and (8f.2)
AnisotropicMinimumDissipation with constant Poincaré coefficients (…/anisotropic_minimum_dissipation.jl), and Smagorinsky /
SmagorinskyLilly with constant coefficients (…/Smagorinskys/smagorinsky.jl, lilly_coefficient.jl)."""
import ctypes as C

import numpy as np


class ExplicitTimeDiscretization:
    """A fully-explicit time-discretization of a TurbulenceClosure (implicit_explicit_time_discretization.jl:5-12)."""

    def __repr__(self):
        return "ExplicitTimeDiscretization"

    def __eq__(self, other):
        return type(other) is type(self)

    __hash__ = object.__hash__


class VerticallyImplicitTimeDiscretization(ExplicitTimeDiscretization):
    """A vertically-implicit time-discretization of a TurbulenceClosure (implicit_explicit_time_discretization.jl:14-28):
    [∇ ⋅ q]ⁿ = [explicit_flux_divergence]ⁿ + [∂z (κ ∂z c)]ⁿ⁺¹, the implicit part solved after every substep (implicit_step!)."""

    def __repr__(self):
        return "VerticallyImplicitTimeDiscretization"


def _is_time_discretization(x):
    return isinstance(x, ExplicitTimeDiscretization) or (isinstance(x, type) and issubclass(x, ExplicitTimeDiscretization))


def _time_discretization(td):
    if isinstance(td, type) and issubclass(td, ExplicitTimeDiscretization):
        td = td()
    if not isinstance(td, ExplicitTimeDiscretization):
        raise TypeError("time_discretization must be ExplicitTimeDiscretization() or VerticallyImplicitTimeDiscretization()")
    return td


def is_vertically_implicit(closure):
    """is_vertically_implicit(closure) (vertically_implicit_diffusion_solver.jl:178)"""
    return isinstance(getattr(closure, "time_discretization", None), VerticallyImplicitTimeDiscretization)


class ScalarDiffusivity:
    """ScalarDiffusivity(time_discretization = ExplicitTimeDiscretization(), ν = 0, κ = 0) (scalar_diffusivity.jl:21-141): the time
    discretisation is the first positional argument or a keyword; a number in first position is ν. κ a number (all tracers) or a dict
    tracer-name -> number."""

    def __init__(self, *args, ν=0.0, κ=0.0, nu=None, kappa=None, time_discretization=None):
        args = list(args)
        if args and _is_time_discretization(args[0]):
            if time_discretization is not None:
                raise TypeError("time_discretization given twice")
            time_discretization = args.pop(0)
        if len(args) > 2:
            raise TypeError("ScalarDiffusivity([time_discretization,] ν, κ)")
        if args:
            ν = args.pop(0)
        if args:
            κ = args.pop(0)
        self.time_discretization = _time_discretization(ExplicitTimeDiscretization() if time_discretization is None else time_discretization)
        ν = ν if nu is None else nu
        κ = κ if kappa is None else kappa
        if callable(ν) or callable(κ) or (isinstance(κ, dict) and any(callable(x) for x in κ.values())):
            raise NotImplementedError("only constant (Number) viscosity / diffusivity is on the accelerated path")
        self.ν, self.κ = float(ν), ({n: float(v) for n, v in κ.items()} if isinstance(κ, dict) else float(κ))   # convert_diffusivity(FT, κ)
        if self.ν < 0:
            raise ValueError("viscosity must be non-negative")

    def kappa_array(self, tracer_names):
        if isinstance(self.κ, dict):
            missing = [n for n in tracer_names if n not in self.κ]
            if missing:
                raise ValueError(f"κ is missing tracers {missing}")     # with_tracers(), scalar_diffusivity.jl:151-160
            vals = [float(self.κ[n]) for n in tracer_names]
        else:
            vals = [float(self.κ)] * len(tracer_names)
        if any(v < 0 for v in vals):
            raise ValueError("diffusivity must be non-negative")
        arr = np.ascontiguousarray(vals if vals else [0.0], dtype=np.float64)
        return arr, arr.ctypes.data_as(C.POINTER(C.c_double))

    def __repr__(self):
        return f"ScalarDiffusivity{{{self.time_discretization!r}}}(ν={self.ν}, κ={self.κ})"


def VerticalScalarDiffusivity(*args, **kwargs):
    """VerticalScalarDiffusivity(...) (scalar_diffusivity.jl:120-121): named so that it can be refused -- the vertical formulation needs its
    own explicit flux kernels"""
    raise NotImplementedError("VerticalScalarDiffusivity is not on the accelerated path: only the isotropic ScalarDiffusivity is")


def _refuse_vertically_implicit(name, time_discretization):
    """the eddy-coefficient closures are accelerated with ExplicitTimeDiscretization only"""
    if time_discretization is not None and isinstance(_time_discretization(time_discretization), VerticallyImplicitTimeDiscretization):
        raise NotImplementedError(f"{name} with VerticallyImplicitTimeDiscretization is not on the accelerated path: its coefficients "
                                  "differ from column to column")


class AnisotropicMinimumDissipation:
    """AnisotropicMinimumDissipation(; C = 1/3, Cν = nothing, Cκ = nothing, Cb = nothing) (anisotropic_minimum_dissipation.jl:128-139):
    Cκ a number (all tracers) or a dict tracer-name -> number. The eddy viscosity / diffusivities are the model's
    `diffusivity_fields` (νₑ, κₑ)."""

    def __init__(self, C=1 / 3, Cν=None, Cκ=None, Cb=None, Cnu=None, Ckappa=None, time_discretization=None):
        if _is_time_discretization(C):                  # AnisotropicMinimumDissipation(time_discretization; C, ...) (:128)
            C, time_discretization = 1 / 3, C
        _refuse_vertically_implicit("AnisotropicMinimumDissipation", time_discretization)
        Cν = Cν if Cnu is None else Cnu
        Cκ = Cκ if Ckappa is None else Ckappa
        if Cb is not None:
            raise NotImplementedError("the (unvalidated) buoyancy modification Cb is not on the accelerated path")
        self.Cν = C if Cν is None else Cν
        self.Cκ = C if Cκ is None else Cκ
        if callable(self.Cν) or callable(self.Cκ) or (isinstance(self.Cκ, dict) and any(callable(x) for x in self.Cκ.values())):
            raise NotImplementedError("only constant (Number) Poincaré coefficients are on the accelerated path")
        self.Cν = float(self.Cν)
        self.Cb = None

    def Ckappa_array(self, tracer_names):
        import ctypes
        if isinstance(self.Cκ, dict):
            missing = [n for n in tracer_names if n not in self.Cκ]
            if missing:
                raise ValueError(f"Cκ is missing tracers {missing}")     # tracer_diffusivities via with_tracers (:141-144)
            vals = [float(self.Cκ[n]) for n in tracer_names]
        else:
            vals = [float(self.Cκ)] * len(tracer_names)
        arr = np.ascontiguousarray(vals if vals else [0.0], dtype=np.float64)
        return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def __repr__(self):
        return f"AnisotropicMinimumDissipation{{ExplicitTimeDiscretization}}(Cν={self.Cν}, Cκ={self.Cκ}, Cb=nothing)"


class _Colon:
    """Julia's `:` as an averaging: all three directions. ocn.Colon (also spelt ":")"""

    def __repr__(self):
        return "Colon()"


Colon = _Colon()


class LagrangianAveraging:
    """LagrangianAveraging() (Smagorinskys/dynamic_coefficient.jl:32): 𝒥ᴸᴹ and 𝒥ᴹᴹ are averaged along fluid-parcel trajectories"""

    def __repr__(self):
        return "LagrangianAveraging()"

    def __eq__(self, other):
        return type(other) is type(self)

    __hash__ = object.__hash__


def _averaging(averaging):
    """the averaging as the reference holds it -- an Int, a tuple of Ints, Colon or LagrangianAveraging() -- and the library's mask of the
    averaged directions (bit d: direction d + 1; 0: Lagrangian)"""
    if isinstance(averaging, LagrangianAveraging) or averaging is LagrangianAveraging:
        return LagrangianAveraging(), 0
    if averaging is Colon or (isinstance(averaging, str) and averaging == ":"):
        return Colon, 7
    if isinstance(averaging, bool):
        raise TypeError("averaging is an Int, a tuple of Ints out of (1, 2, 3), Colon or LagrangianAveraging()")
    if isinstance(averaging, (int, np.integer)):
        dims, kept = (int(averaging),), int(averaging)
    elif isinstance(averaging, (tuple, list)) and averaging and all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) for d in averaging):
        dims = tuple(int(d) for d in averaging)
        kept = dims
    else:
        raise TypeError("averaging is an Int, a tuple of Ints out of (1, 2, 3), Colon or LagrangianAveraging()")
    if any(d not in (1, 2, 3) for d in dims) or len(set(dims)) != len(dims):
        raise ValueError(f"averaging = {averaging}: the directions are distinct and out of (1, 2, 3)")
    return kept, sum(1 << (d - 1) for d in dims)


class DynamicCoefficient:
    """DynamicCoefficient(; averaging, schedule = IterationInterval(1), minimum_numerator = 1e-32) (Smagorinskys/dynamic_coefficient.jl:
    39-117): the scale-invariant dynamic Smagorinsky coefficient of Bou-Zeid et al. (2005). `averaging`: an Int or a tuple of Ints out of
    (1, 2, 3), Colon (all three), or LagrangianAveraging(). `schedule`: an IterationInterval. A DynamicCoefficient without `averaging` can be
    written down (the reference's keyword is required) but no closure takes it."""

    def __init__(self, *args, averaging=None, schedule=None, minimum_numerator=1e-32, **kwargs):
        self.args, self.kwargs = args, kwargs
        self.averaging, self.averaging_mask = (None, None) if averaging is None else _averaging(averaging)
        from .simulations import IterationInterval
        self.schedule = IterationInterval(1) if schedule is None else schedule
        if callable(minimum_numerator):
            raise NotImplementedError("minimum_numerator is a number")
        self.minimum_numerator = float(minimum_numerator)

    def _schedule_text(self):
        s = self.schedule
        return f"IterationInterval({s.interval}, {s.offset})" if hasattr(s, "interval") and hasattr(s, "offset") else repr(s)

    def summary(self):
        """Base.summary (dynamic_coefficient.jl:119)"""
        return f"DynamicCoefficient(averaging = {self.averaging!r}, schedule = {self._schedule_text()})"

    def __repr__(self):
        """Base.show (dynamic_coefficient.jl:120-123)"""
        from .forcings import _jl
        return ("DynamicCoefficient with\n"
                f"├── averaging = {self.averaging!r}\n"
                f"├── schedule = {self._schedule_text()}\n"
                f"└── minimum_numerator = {_jl(self.minimum_numerator)}")


class Smagorinsky:
    """Smagorinsky(; coefficient = 0.16, Pr = 1.0) (Smagorinskys/smagorinsky.jl:62-83): νₑ = (C Δᶠ)² sqrt(2 Σ²), the tracers' diffusivity
    is νₑ / Pr at their flux points. Pr a number (all tracers) or a dict tracer-name -> number. The eddy viscosity is the model's
    `diffusivity_fields.νₑ`."""

    buffer = 2                          # AbstractScalarDiffusivity{TD, ThreeDimensionalFormulation, 2}: required halo size (smagorinsky.jl:11)
    lilly = False
    Cb = 0.0

    def __init__(self, coefficient=0.16, Pr=1.0, time_discretization=None):
        if _is_time_discretization(coefficient):        # Smagorinsky(time_discretization; coefficient, Pr) (smagorinsky.jl:62)
            coefficient, time_discretization = 0.16, coefficient
        _refuse_vertically_implicit(type(self).__name__, time_discretization)
        self.dynamic = isinstance(coefficient, DynamicCoefficient)
        if self.dynamic:
            if self.lilly:
                raise NotImplementedError("the Lilly stability function with a DynamicCoefficient is not a closure of the reference")
            if coefficient.averaging is None:
                raise NotImplementedError("DynamicCoefficient: the keyword `averaging` is required (an Int, a tuple of Ints, Colon or "
                                          "LagrangianAveraging())")
            from .simulations import IterationInterval
            if not isinstance(coefficient.schedule, IterationInterval):
                raise NotImplementedError("the schedule of a DynamicCoefficient on the accelerated path is an IterationInterval")
            if coefficient.schedule.interval < 1:
                raise ValueError("the interval of the schedule must be positive")
        elif callable(coefficient):
            raise NotImplementedError("only a constant (Number) or a DynamicCoefficient Smagorinsky coefficient is on the accelerated path")
        if callable(Pr) or (isinstance(Pr, dict) and any(callable(x) for x in Pr.values())):
            raise NotImplementedError("only constant (Number) Prandtl numbers are on the accelerated path")
        self.coefficient = coefficient if self.dynamic else float(coefficient)
        self.Pr = {n: float(v) for n, v in Pr.items()} if isinstance(Pr, dict) else float(Pr)
        if not self.dynamic and self.coefficient < 0:
            raise ValueError("the Smagorinsky coefficient must be non-negative")
        if any(not v > 0 for v in (self.Pr.values() if isinstance(self.Pr, dict) else [self.Pr])):
            raise ValueError("the Prandtl number must be positive")

    def Pr_array(self, tracer_names):
        if isinstance(self.Pr, dict):
            missing = [n for n in tracer_names if n not in self.Pr]
            if missing:
                raise ValueError(f"Pr is missing tracers {missing}")     # tracer_diffusivities via with_tracers (smagorinsky.jl:87-90)
            vals = [self.Pr[n] for n in tracer_names]
        else:
            vals = [self.Pr] * len(tracer_names)
        arr = np.ascontiguousarray(vals if vals else [1.0], dtype=np.float64)
        return arr, arr.ctypes.data_as(C.POINTER(C.c_double))

    def summary(self):
        """Base.summary (smagorinsky.jl:145)"""
        coefficient = self.coefficient.summary() if self.dynamic else self.coefficient
        return f"Smagorinsky with coefficient = {coefficient}, Pr={self.Pr}"

    def __repr__(self):
        if self.dynamic:                # Base.show (smagorinsky.jl:146-151)
            return f"Smagorinsky closure with\n├── coefficient = {self.coefficient.summary()}\n└── Pr = {self.Pr}"
        return f"Smagorinsky closure with coefficient = {self.coefficient}, Pr = {self.Pr}"


def DynamicSmagorinsky(time_discretization=None, averaging=None, Pr=1.0, schedule=None, minimum_numerator=1e-32):
    """DynamicSmagorinsky(; averaging, Pr = 1.0, schedule = IterationInterval(1), minimum_numerator = 1e-32) (Smagorinskys/
    dynamic_coefficient.jl:20-26): Smagorinsky(coefficient = DynamicCoefficient(averaging, schedule, minimum_numerator), Pr)"""
    if averaging is None:
        raise TypeError("DynamicSmagorinsky: the keyword `averaging` is required")
    return Smagorinsky(coefficient=DynamicCoefficient(averaging=averaging, schedule=schedule, minimum_numerator=minimum_numerator), Pr=Pr,
                       time_discretization=time_discretization)


class SmagorinskyLilly(Smagorinsky):
    """SmagorinskyLilly(; C = 0.16, Cb = 1.0, Pr = 1.0) (Smagorinskys/lilly_coefficient.jl:5-35): the Smagorinsky coefficient reduced by the
    stability function sqrt(1 - Cb N² / Σ²) where the stratification is stable; the buoyancy is the model's."""

    lilly = True

    def __init__(self, C=0.16, Cb=1.0, Pr=1.0, time_discretization=None):
        if _is_time_discretization(C):
            C, time_discretization = 0.16, C
        if callable(Cb):
            raise NotImplementedError("only a constant (Number) reduction factor Cb is on the accelerated path")
        super().__init__(coefficient=C, Pr=Pr, time_discretization=time_discretization)
        self.Cb = float(Cb)

    def __repr__(self):
        return (f"Smagorinsky closure with coefficient = LillyCoefficient(smagorinsky = {self.coefficient}, reduction_factor = {self.Cb}), "
                f"Pr = {self.Pr}")
