"""background_fields of NonhydrostaticModel (reference: src/Models/NonhydrostaticModels/background_fields.jl).

A background field Φ̄ enters the tendencies through advection only (BackgroundFields{false}):

    G_φ = - div(advection, U + Ū, φ) - div(advection, U, Φ̄) + ...

Regularisation (background_fields.jl:97-116) happens on the host, on grid metadata, before the model touches the device: a function
becomes the FunctionField{LX, LY, LZ} it would be in the reference, evaluated once at the nodes of the WHOLE parent array -- halo
values are the function's analytic continuation beyond the domain, never a periodic wrap or a boundary-condition fill --, a number a
ConstantField, a Field stays the caller's array (its halos are whatever the caller put there). Only time-independent backgrounds are
served: the arrays are uploaded once."""
import inspect
from collections import namedtuple

import numpy as np

from .fields import Field
from .grids import Center, Face

VELOCITY_LOCATIONS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}


class BackgroundField:
    """BackgroundField(func; parameters=nothing) (background_fields.jl:66-91): func(x, y, z, t) or func(x, y, z, t, parameters);
    func(x, y, z) is accepted too, and a number is a ConstantField"""

    def __init__(self, func, parameters=None):
        self.func, self.parameters = func, parameters

    def __repr__(self):
        return f"BackgroundField\n├── func: {getattr(self.func, '__name__', self.func)}\n└── parameters: {self.parameters}"


class BackgroundFields:
    """BackgroundFields(; background_closure_fluxes=false, fields...) (background_fields.jl:32-54). After regularisation `velocities`
    and `tracers` are namedtuples whose entries are host parent arrays, Fields, or None (ZeroField); the model replaces them by Fields."""

    def __init__(self, background_closure_fluxes=False, **fields):
        self.background_closure_fluxes = bool(background_closure_fluxes)
        self.fields = dict(fields)
        self.velocities = self.tracers = None


def _loc_names(loc):
    return "(" + ", ".join(l.__name__ for l in loc) + ")"


def parent_nodes(grid, loc):
    """the node coordinates of every index of the parent array of a field at `loc`, halos included, as broadcastable arrays"""
    F = (grid.xᶠᵃᵃ, grid.yᵃᶠᵃ, grid.zᵃᵃᶠ)
    Cn = (grid.xᶜᵃᵃ, grid.yᵃᶜᵃ, grid.zᵃᵃᶜ)
    shape_of = grid.total_size(loc)
    out = []
    for d in range(3):
        a = np.asarray(F[d] if loc[d] is Face else Cn[d], dtype=np.float64)[:shape_of[d]]
        if a.shape != (shape_of[d],):
            raise ValueError(f"grid has {a.shape[0]} nodes along dimension {d}, the parent array {shape_of[d]}")
        shape = [1, 1, 1]
        shape[d] = shape_of[d]
        out.append(a.reshape(shape))
    return out


def _call(func, parameters, x, y, z, t):
    if parameters is not None:
        return func(x, y, z, t, parameters)
    try:
        nargs = len([p for p in inspect.signature(func).parameters.values()
                     if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) and p.default is p.empty])
    except (TypeError, ValueError):
        nargs = 4
    return func(x, y, z) if nargs == 3 else func(x, y, z, t)


def _evaluate(func, parameters, grid, loc, time):
    x, y, z = parent_nodes(grid, loc)
    shape = grid.total_size(loc)

    def at(t):
        return np.asfortranarray(np.broadcast_to(np.asarray(_call(func, parameters, x, y, z, t), dtype=np.float64), shape))
    a, b = at(time), at(time + 1.0)
    if not np.array_equal(a, b, equal_nan=True):
        raise NotImplementedError("time dependence of a background field is not served: the function is evaluated once, when the model "
                                  "is built (its values at the clock's time and one time unit later differ)")
    return a


def regularize_background_field(loc, value, grid, time=0.0):
    """regularize_background_field(LX, LY, LZ, f, grid, clock) (background_fields.jl:97-116): a host parent array (Fortran order), the
    Field itself, or None"""
    if value is None:
        return None
    if isinstance(value, Field):
        if tuple(value.loc) != tuple(loc):
            raise ValueError(f"Cannot use field at {_loc_names(value.loc)} as a background field at {_loc_names(loc)}")
        if value.shape != grid.total_size(loc):
            raise ValueError(f"background field of parent size {value.shape} on a grid whose fields have {grid.total_size(loc)}")
        return value
    func, parameters = (value.func, value.parameters) if isinstance(value, BackgroundField) else (value, None)
    shape = grid.total_size(loc)
    if isinstance(func, np.ndarray):
        if func.shape != shape:
            raise ValueError(f"a background array has the parent size {shape} of its field (halos included), got {func.shape}")
        return np.asfortranarray(func, dtype=np.float64)
    if callable(func):
        return _evaluate(func, parameters, grid, loc, time)
    if isinstance(func, (int, float, np.integer, np.floating)) and not isinstance(func, bool):
        return np.full(shape, float(func), dtype=np.float64, order="F")                 # ConstantField
    raise ValueError(f"a background field is a BackgroundField, a function, a number, a Field or a parent-shaped array; got {type(func).__name__}")


def regularize_background_fields(background_fields, tracer_names, grid, time=0.0):
    """BackgroundFields(background_fields, tracer_names, grid, clock) (background_fields.jl:56-66). Raises before anything touches the
    device; returns None for no background fields at all."""
    if background_fields is None:
        return None
    if isinstance(background_fields, BackgroundFields):
        if background_fields.background_closure_fluxes:
            raise NotImplementedError("BackgroundFields(background_closure_fluxes=true) is not served: closures see the model's own fields only")
        given = dict(background_fields.fields)
    else:
        given = dict(background_fields)
    if not given:
        return None
    if hasattr(grid, "local"):
        raise NotImplementedError("background_fields are not served on a partitioned grid")
    tracer_names = tuple(tracer_names)
    for name in given:
        if name not in VELOCITY_LOCATIONS and name not in tracer_names:
            raise ValueError(f"background field given for {name}, which is not a velocity or tracer of the model")
    out = BackgroundFields()
    out.fields = given
    V = namedtuple("BackgroundVelocities", "u v w")
    out.velocities = V(*[regularize_background_field(VELOCITY_LOCATIONS[n], given.get(n), grid, time) for n in "uvw"])
    T = namedtuple("BackgroundTracers", tracer_names) if tracer_names else tuple
    ccc = (Center, Center, Center)
    out.tracers = T(*[regularize_background_field(ccc, given.get(n), grid, time) for n in tracer_names])
    return out


def empty_background_fields(tracer_names):
    """what a model without the keyword carries: every velocity and tracer background None (the reference's ZeroFields)"""
    out = BackgroundFields()
    out.velocities = namedtuple("BackgroundVelocities", "u v w")(None, None, None)
    tracer_names = tuple(tracer_names)
    out.tracers = namedtuple("BackgroundTracers", tracer_names)(*[None] * len(tracer_names)) if tracer_names else tuple()
    return out


def upload(model, regularized):
    """hand the regularised backgrounds to the library (ocn_model_set_background_field); host arrays become device Fields the model owns.
    Returns the BackgroundFields whose entries are Fields or None."""
    from . import _lib
    grid = model.grid

    def field_of(loc, value):
        if value is None or isinstance(value, Field):
            return value
        f = Field(loc, grid)
        f.set_parent(value)
        return f
    V = type(regularized.velocities)
    vel = V(*[field_of(VELOCITY_LOCATIONS[n], v) for n, v in zip("uvw", regularized.velocities)])
    ccc = (Center, Center, Center)
    tr = [field_of(ccc, v) for v in regularized.tracers]
    T = type(regularized.tracers)
    regularized.velocities, regularized.tracers = vel, (T(*tr) if model.tracer_names else tuple())
    for cname, f in list(zip("uvw", vel)) + [("c%d" % n, f) for n, f in enumerate(tr)]:
        if f is not None:
            _lib.check(_lib.lib().ocn_model_set_background_field(model.handle, cname.encode(), f.data))
    return regularized
