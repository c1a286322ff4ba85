"""Boundary conditions (reference: src/BoundaryConditions/boundary_condition.jl, boundary_condition_classifications.jl,
field_boundary_conditions.jl, continuous_boundary_function.jl). A condition is a number, a 2-D array over the boundary, a LinearFieldFlux,
or -- Flux conditions only -- a function: FluxBoundaryCondition(func, field_dependencies=..., parameters=...) with the reference's
signature func(X..., t, deps..., [parameters]). The model records the function's operations once and evaluates them on the device at every
boundary point before each use of the Flux conditions (boundary_functions.py). Functions in Value / Gradient / Open conditions,
discrete_form=True, functions on diffusivity fields, on partitioned grids and in a free-standing fill are refused by name."""
import ctypes as C

import numpy as np

from . import _lib

SIDES = ("west", "east", "south", "north", "bottom", "top")
KINDS = {"Default": 0, "Flux": 1, "Value": 2, "Gradient": 3, "Open": 4}


class LinearFieldFlux:
    """the boundary function (ξ, η, t, φ, p) -> a + b φ of one field dependency φ: the family of field-dependent Flux conditions that
    crosses the C ABI (ocn_model_set_linear_flux_bc). Jˢ(x, y, t, S, rate) = -rate S of examples/ocean_wind_mixing_and_convection.jl:
    125 is LinearFieldFlux(b=-rate)."""

    def __init__(self, a=0.0, b=0.0):
        self.a, self.b = float(a), float(b)


class PerturbationAdvection:
    """PerturbationAdvection(; inflow_timescale = 0, outflow_timescale = Inf) (perturbation_advection.jl:4-7,57-63): the scheme of a
    radiating OpenBoundaryCondition -- the boundary value is advected out with the exterior value ū and relaxed to it over
    inflow_timescale where ū points into the domain and over outflow_timescale where it points out. Positionally the fields come in the
    struct's order, inflow before outflow."""

    def __init__(self, inflow_timescale=0, outflow_timescale=float("inf")):
        self.inflow_timescale, self.outflow_timescale = float(inflow_timescale), float(outflow_timescale)          # convert(FT, ...)
        if not (self.inflow_timescale >= 0 and self.outflow_timescale >= 0):
            raise ValueError("PerturbationAdvection timescales must be non-negative")

    def __repr__(self):
        from .forcings import _jl
        return f"PerturbationAdvection{{Float64}}({_jl(self.inflow_timescale)}, {_jl(self.outflow_timescale)})"

    def __eq__(self, other):
        return (isinstance(other, PerturbationAdvection) and
                (self.inflow_timescale, self.outflow_timescale) == (other.inflow_timescale, other.outflow_timescale))

    __hash__ = None


class BoundaryCondition:
    """BoundaryCondition(classification, condition::Number); Flux conditions also take a LinearFieldFlux with field_dependencies; Open
    conditions a scheme (Open(scheme), boundary_condition_classifications.jl:70-72)"""

    def __init__(self, classification, condition=0.0, field_dependencies=None, scheme=None, parameters=None, discrete_form=False):
        if classification not in KINDS:
            raise ValueError(f"unknown boundary condition classification {classification}")
        if scheme is not None and classification != "Open":
            raise ValueError("only an Open boundary condition carries a scheme")
        if scheme is not None and not isinstance(scheme, PerturbationAdvection):
            raise NotImplementedError("scheme must be nothing or PerturbationAdvection(inflow_timescale, outflow_timescale)")
        self.scheme = scheme
        self.linear = None
        self.function = None
        if discrete_form:
            raise NotImplementedError("discrete_form=True (a DiscreteBoundaryFunction indexes the fields itself) is not built: write the "
                                      "condition in the continuous form func(X..., t, deps..., [parameters])")
        if callable(condition) and not isinstance(condition, LinearFieldFlux) and classification == "Flux":
            from .boundary_functions import ContinuousBoundaryFunction
            self.function = ContinuousBoundaryFunction(condition, parameters, field_dependencies)
            condition = 0.0
        if isinstance(condition, LinearFieldFlux):
            deps = (field_dependencies,) if isinstance(field_dependencies, str) else tuple(field_dependencies or ())
            if classification != "Flux" or len(deps) != 1:
                raise NotImplementedError("a LinearFieldFlux is a Flux condition with exactly one field dependency")
            self.linear = (condition.a, condition.b, str(deps[0]).lstrip(":"))
            condition = 0.0
        self.array = None
        if isinstance(condition, np.ndarray) or (isinstance(condition, (list, tuple)) and np.ndim(condition) == 2):
            # getbc(condition::AbstractArray, i, j, grid, args...) = condition[i, j] (boundary_condition.jl:164): a 2-D array over the
            # interior extents of the two tangential directions, uploaded once and handed to the library as a device pointer
            self.array = np.asfortranarray(condition, dtype=np.float64)
            if self.array.ndim != 2:
                raise ValueError("an array-valued boundary condition is a 2-D array over the two tangential directions")
            self._device = None
            condition = 0.0
        if callable(condition):
            raise NotImplementedError(f"a function in a {classification} condition is not built (it would have to be evaluated before every "
                                      "halo fill): only constant (Number) or array boundary conditions are on the accelerated path there; "
                                      "Flux conditions take functions")
        if not isinstance(condition, (int, float)):
            raise NotImplementedError("only constant (Number) or array boundary conditions, LinearFieldFlux and (Flux) functions are on the accelerated path")
        self.classification, self.condition = classification, float(condition)

    def device_array(self, expected_shape=None):
        """device copy of an array-valued condition (None for a number), created on first use and freed with the condition"""
        if self.array is None:
            return None
        if expected_shape is not None and tuple(self.array.shape) != tuple(expected_shape):
            raise ValueError(f"boundary condition array has shape {self.array.shape}, the boundary has {tuple(expected_shape)} points")
        if self._device is None:
            p = C.c_void_p()
            _lib.check(_lib.lib().ocn_malloc(C.byref(p), self.array.nbytes))
            _lib.check(_lib.lib().ocn_memcpy_h2d(p, self.array.ctypes.data_as(C.c_void_p), self.array.nbytes))
            self._device = p
        return self._device

    def __del__(self):
        try:
            if getattr(self, "_device", None) is not None:
                _lib.lib().ocn_free(self._device)
        except Exception:
            pass

    def __repr__(self):
        if self.scheme is not None:
            return f"OpenBoundaryCondition: {self.condition if self.array is None else 'Array'} with {self.scheme!r}"
        if self.linear:
            return f"FluxBoundaryCondition: {self.linear[0]} + {self.linear[1]} * {self.linear[2]}"
        if self.function is not None:
            return f"FluxBoundaryCondition: {self.function!r}"
        if self.array is not None:
            return f"{self.classification}BoundaryCondition: {self.array.shape[0]}×{self.array.shape[1]} Array{{Float64, 2}}"
        return f"{self.classification}BoundaryCondition: {self.condition}"


def FluxBoundaryCondition(value, field_dependencies=None, parameters=None, discrete_form=False):
    """FluxBoundaryCondition(Number | array) | FluxBoundaryCondition(LinearFieldFlux(a, b), field_dependencies = :φ) |
    FluxBoundaryCondition(func, field_dependencies = (...), parameters = p) with func(X..., t, deps..., [p]) (boundary_functions.py)"""
    return BoundaryCondition("Flux", value, field_dependencies, parameters=parameters, discrete_form=discrete_form)


def ValueBoundaryCondition(value):
    return BoundaryCondition("Value", value)


def GradientBoundaryCondition(value):
    return BoundaryCondition("Gradient", value)


def OpenBoundaryCondition(value, scheme=None):
    """OpenBoundaryCondition(val; scheme = nothing) (boundary_condition.jl:108)"""
    return BoundaryCondition("Open", value, scheme=scheme)


def scheme_sides(fbcs):
    """the sides of a FieldBoundaryConditions (or None) whose Open condition carries a scheme"""
    return [s for s, bc in fbcs.sides.items() if bc.scheme is not None] if fbcs is not None else []


def validate_open_boundary_schemes(boundary_conditions, grid):
    """a scheme is accepted where the reference has a method for it: on the wall-normal velocity of a Bounded direction (_fill_west_halo!
    .. _fill_top_halo! for a PAOBC, perturbation_advection.jl:119-180: u west / east, v south / north, w bottom / top), on one device.
    Raises NotImplementedError otherwise -- called before anything touches the device."""
    from .grids import Bounded
    normal = {"u": ("west", "east"), "v": ("south", "north"), "w": ("bottom", "top")}
    for name, fbcs in dict(boundary_conditions or {}).items():
        if not isinstance(fbcs, FieldBoundaryConditions):
            continue
        for side in scheme_sides(fbcs):
            if hasattr(grid, "local"):
                raise NotImplementedError("an OpenBoundaryCondition with a scheme is not served on partitioned grids")
            if side not in normal.get(name, ()):
                raise NotImplementedError(f"a scheme belongs to the wall-normal velocity of its side (u west / east, v south / north, "
                                          f"w bottom / top); got {name}.{side}")
            if grid.topology[SIDES.index(side) // 2] is not Bounded:
                raise NotImplementedError(f"a scheme needs a Bounded direction; {name}.{side} is not on one")


def function_sides(fbcs):
    """the sides of a FieldBoundaryConditions (or None) whose Flux condition is a function"""
    return [s for s, bc in fbcs.sides.items() if bc.function is not None] if isinstance(fbcs, FieldBoundaryConditions) else []


def validate_boundary_functions(boundary_conditions, grid):
    """function-valued Flux conditions are served for the velocities and tracers of a model on one device. Raises NotImplementedError
    otherwise -- called before anything touches the device."""
    import unicodedata
    for name, fbcs in dict(boundary_conditions or {}).items():
        diffusivity = unicodedata.normalize("NFKC", name) in ("νe", "nu_e", "κe", "kappa_e")
        nested = list(dict(fbcs).values()) if diffusivity and not isinstance(fbcs, FieldBoundaryConditions) else [fbcs]
        for entry in nested:
            if not function_sides(entry):
                continue
            if diffusivity:
                raise NotImplementedError(f"a function-valued condition of the diffusivity field {name} is not built")
            if hasattr(grid, "local"):
                raise NotImplementedError("a function-valued boundary condition is not served on partitioned grids")


class FieldBoundaryConditions:
    """FieldBoundaryConditions(; west, east, south, north, bottom, top): unspecified sides keep the defaults of
    field_boundary_conditions.jl:15-25 (Periodic -> periodic, Bounded + Center -> no flux, Bounded + Face -> impenetrable)"""

    def __init__(self, **sides):
        if sides.pop("immersed", None) is not None:
            # FieldBoundaryConditions(immersed = ...) (field_boundary_conditions.jl, immersed_boundary_condition.jl)
            from .immersed_boundaries import refuse
            refuse("FieldBoundaryConditions(immersed=...) (a boundary condition on the immersed boundary)")
        for s, bc in sides.items():
            if s not in SIDES:
                raise ValueError(f"unknown side {s}; expected one of {SIDES}")
            if bc is not None and not isinstance(bc, BoundaryCondition):
                raise TypeError(f"{s} must be a BoundaryCondition")
        self.sides = {s: bc for s, bc in sides.items() if bc is not None}

    def c_array(self, grid=None):
        arr = (_lib.BC * 6)()
        if scheme_sides(self):
            # step_left_boundary! / step_right_boundary! read clock.last_stage_Δt: a fill without a model has no clock
            raise NotImplementedError("an OpenBoundaryCondition with a scheme is stepped with the model's clock: it is a model boundary "
                                      "condition, not one of a free-standing fill or flux computation")
        for s, bc in self.sides.items():
            if bc.function is not None:
                # getbc(::ContinuousBoundaryFunction, ..., clock, model_fields): a fill without a model has neither
                raise NotImplementedError("a function-valued boundary condition is evaluated with the model's clock and fields: it is a model "
                                          "boundary condition, not one of a free-standing fill or flux computation")
            q = SIDES.index(s)
            arr[q].kind = KINDS[bc.classification]
            arr[q].value = bc.condition
            if bc.array is not None:
                arr[q].array = bc.device_array(_tangential_shape(grid, q) if grid is not None else None)
        arr._keep = self                    # the device arrays live as long as the conditions
        return arr


def _tangential_shape(grid, side):
    """interior extents of the two tangential directions of side 0..5 (west, east, south, north, bottom, top), x before y before z"""
    N = grid.size
    d = side // 2
    return (N[1], N[2]) if d == 0 else ((N[0], N[2]) if d == 1 else (N[0], N[1]))


def bc_table(fields_bcs, grid=None):
    """list of FieldBoundaryConditions | None, one per field -> ocn_bc_t[n][6]"""
    table = ((_lib.BC * 6) * len(fields_bcs))()
    table._keep = list(fields_bcs)
    for f, fb in enumerate(fields_bcs):
        if fb is not None:
            row = fb.c_array(grid)
            for s in range(6):
                table[f][s].kind, table[f][s].value, table[f][s].array = row[s].kind, row[s].value, row[s].array
    return table


def compute_flux_bcs(G, bcs):
    """compute_x_bcs! / compute_y_bcs! / compute_z_bcs! (compute_flux_bcs.jl:12-163) on the tendency field G"""
    loc = (C.c_int * 3)(*[1 if l.__name__ == "Face" else 0 for l in G.loc])
    _lib.check(_lib.lib().ocn_compute_flux_bcs(G.grid.handle, G.data, loc, bcs.c_array(G.grid)))
