"""Forcings (reference: src/Forcings/): the closure-free forcings a model's tendencies can carry -- Relaxation with GaussianMask /
PiecewiseLinearMask / LinearTarget, Forcing(array) and MultipleForcings -- and `model_forcing`, which regularises the `forcing = (...)`
of the model constructor into the per-field term descriptors of ocn_model_set_forcing (include/ocn_mi355x.h).

The built-in masks and targets depend on one coordinate and not on time, so they are evaluated HERE, on the host, at the forced field's own
nodes (the grid's node arrays with halos, `xᶠᵃᵃ / xᶜᵃᵃ / ...`); the device does the `*` and `-` of relaxation.jl per cell (ocn_forcing.h).

A `mask(x, y, z)` or `target(x, y, z, t)` that is a function of the user's makes the whole relaxation ONE recorded program
(boundary_functions.py), `rate * mask(X...) * (target(X..., t) - φ)`, evaluated on the device at every cell (ocn_forcing_function.h):

    sponge = Relaxation(rate=1 / 60, mask=lambda x, y, z: ocn.max_(west(x), bottom(z)), target=lambda x, y, z, t: T0 + A * ocn.sin(ω * t))"""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Center, Face, Flat

_DIRS = ("x", "y", "z")


def _jl(v):
    """Julia's print of a Number (Int64 / Float64): 100 -> "100", 100.0 -> "100.0", 1e-06 -> "1.0e-6" """
    if isinstance(v, (bool, np.bool_)):
        return "true" if v else "false"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    s = repr(float(v))
    if s in ("inf", "-inf", "nan"):
        return {"inf": "Inf", "-inf": "-Inf", "nan": "NaN"}[s]
    if "e" in s:
        m, e = s.split("e")
        if "." not in m:
            m += ".0"
        return m + "e" + str(int(e))
    return s


def _jl_type(v):
    return "Int64" if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else "Float64"


def _promote(a, b):
    """promote_type of two Numbers (Int64, Float64)"""
    if _jl_type(a) == "Int64" and _jl_type(b) == "Int64":
        return int(a), int(b)
    return float(a), float(b)


def _direction(D):
    D = str(D).lstrip(":")
    if D not in _DIRS:
        raise ValueError(f"direction must be :x, :y or :z, got {D!r}")
    return D


class _Directional:
    """`Name{D}(; ...)` is written `Name["z"](...)` or `Name("z", ...)`"""

    def __class_getitem__(cls, D):
        return lambda **kw: cls(D, **kw)


def onefunction(*args):
    return 1


def zerofunction(*args):
    return 0


class GaussianMask(_Directional):
    """GaussianMask{D}(; center, width) (relaxation.jl): exp(-(D - center)^2 / (2 * width^2))"""

    def __init__(self, D, center, width):
        self.D = _direction(D)
        self.center, self.width = _promote(center, width)

    def __call__(self, xi):
        d = np.asarray(xi, dtype=np.float64) - self.center
        # `(ξ - center)^2` is the literal power ξ * ξ; `2 * width^2` in the promoted type (Int64 stays exact)
        return np.exp(-(d * d) / (2 * (self.width * self.width)))

    def summary(self):
        c = self.center
        arg = f"{self.D}^2" if c == 0 else (f"({self.D} - {_jl(c)})^2" if c > 0 else f"({self.D} + {_jl(-c)})^2")
        return f"exp(-{arg} / (2 * {_jl(self.width)}^2))"

    def __repr__(self):
        return f"GaussianMask{{:{self.D}, {_jl_type(self.center)}}}({_jl(self.center)}, {_jl(self.width)})"


class PiecewiseLinearMask(_Directional):
    """PiecewiseLinearMask{D}(; center, width) (relaxation.jl): max(0, 1 - abs(D - center) / width)"""

    def __init__(self, D, center, width):
        self.D = _direction(D)
        self.center, self.width = _promote(center, width)

    def __call__(self, xi):
        d = 1.0 - np.abs(np.asarray(xi, dtype=np.float64) - self.center) / self.width
        return np.maximum(0.0, d)

    def summary(self):
        return f"piecewise_linear({self.D}, center={_jl(self.center)}, width={_jl(self.width)})"

    def __repr__(self):
        return f"PiecewiseLinearMask{{:{self.D}, {_jl_type(self.center)}}}({_jl(self.center)}, {_jl(self.width)})"


class LinearTarget(_Directional):
    """LinearTarget{D}(; intercept, gradient) (relaxation.jl): intercept + gradient * D"""

    def __init__(self, D, intercept, gradient):
        self.D = _direction(D)
        self.intercept, self.gradient = _promote(intercept, gradient)

    def __call__(self, xi):
        return self.intercept + self.gradient * np.asarray(xi, dtype=np.float64)

    def summary(self):
        return f"{_jl(self.intercept)} + {_jl(self.gradient)} * {self.D}"

    def __repr__(self):
        return f"LinearTarget{{:{self.D}, {_jl_type(self.intercept)}}}({_jl(self.intercept)}, {_jl(self.gradient)})"


def _summary(f):
    if f is onefunction:
        return "1"
    if f is zerofunction:
        return "0"
    if isinstance(f, (int, float, np.integer, np.floating)):
        return _jl_type(f)                                  # summary(::Number) is its type
    return f.summary() if hasattr(f, "summary") else repr(f)


def _type_name(f):
    if f is onefunction:
        return "typeof(Oceananigans.Forcings.onefunction)"
    if f is zerofunction:
        return "typeof(Oceananigans.Forcings.zerofunction)"
    if isinstance(f, (int, float, np.integer, np.floating)):
        return _jl_type(f)
    if isinstance(f, (GaussianMask, PiecewiseLinearMask, LinearTarget)):
        return f"{type(f).__name__}{{:{f.D}, {_jl_type(f.center if hasattr(f, 'center') else f.intercept)}}}"
    return type(f).__name__


class Relaxation:
    """Relaxation(; rate, mask=onefunction, target=zerofunction) (relaxation.jl): rate * mask(x, y, z) * (target(x, y, z, t) - φ)"""

    def __init__(self, rate, mask=onefunction, target=zerofunction):
        self.rate, self.mask, self.target = rate, mask, target

    def summary(self):
        return f"Relaxation(rate={_jl(self.rate)}, mask={_summary(self.mask)}, target={_summary(self.target)})"

    def __repr__(self):
        return (f"Relaxation{{{_jl_type(self.rate)}, {_type_name(self.mask)}, {_type_name(self.target)}}}\n"
                f"├── rate: {_jl(self.rate)}\n├── mask: {_summary(self.mask)}\n└── target: {_summary(self.target)}")


class ArrayForcing:
    """Forcing(array) (forcing.jl:165-177): F = array[i, j, k]; `array` has size(grid) -- a numpy array (copied to a device buffer the
    model owns) or a (Center, Center, Center) Field (borrowed: writing it between time-steps changes the forcing)."""

    def __init__(self, array):
        self.array = array

    def summary(self):
        a = self.array
        shape = "×".join(str(n) for n in (a.shape if isinstance(a, np.ndarray) else a.grid.size))
        return f"DiscreteForcing({shape} array)"

    __repr__ = summary


class ContinuousForcing:
    """Forcing(func; parameters, field_dependencies) (continuous_forcing.jl): a Julia closure -- not on the device path"""

    def __init__(self, func, parameters=None, field_dependencies=()):
        self.func, self.parameters, self.field_dependencies = func, parameters, field_dependencies


class DiscreteForcing:
    """Forcing(func; discrete_form = true, parameters) (discrete_forcing.jl): a Julia closure -- not on the device path"""

    def __init__(self, func, parameters=None):
        self.func, self.parameters = func, parameters


class AdvectiveForcing:
    """AdvectiveForcing(; u, v, w) (advective_forcing.jl) -- not on the device path"""

    def __init__(self, u=None, v=None, w=None):
        self.u, self.v, self.w = u, v, w


def Forcing(func, parameters=None, field_dependencies=(), discrete_form=False):
    """Forcing(array) / Forcing(func; parameters, field_dependencies, discrete_form) (forcing.jl)"""
    from .fields import Field
    if isinstance(func, (np.ndarray, Field)):
        return ArrayForcing(func)
    if discrete_form:
        return DiscreteForcing(func, parameters=parameters)
    return ContinuousForcing(func, parameters=parameters, field_dependencies=field_dependencies)


class MultipleForcings:
    """MultipleForcings(f₁, f₂, ...) == MultipleForcings((f₁, f₂, ...)) == (f₁, f₂, ...) (multiple_forcings.jl): F₁ + F₂ + ..."""

    def __init__(self, *forcings):
        if len(forcings) == 1 and isinstance(forcings[0], (tuple, list)):
            forcings = tuple(forcings[0])
        self.forcings = tuple(forcings)

    def __getitem__(self, i):
        return self.forcings[i]

    def __len__(self):
        return len(self.forcings)

    def summary(self):
        n = len(self.forcings)
        return f"MultipleForcings with {n} forcing" + ("s" if n > 1 else "")

    def __repr__(self):
        body = [f"├ {_summary(f)}\n" for f in self.forcings[:-1]] + [f"└ {_summary(self.forcings[-1])}"]
        return self.summary() + ":\n" + "".join(body)


# ---- regularisation: forcing = (name = F,) -> per-field term descriptors ----------------------------------------------------------

def _unsupported(f):
    kind = "a callable (Julia function)" if callable(f) and not isinstance(f, type) else f"type {type(f).__name__}"
    return NotImplementedError(f"forcing of {kind} is outside the accelerated path: only Relaxation (GaussianMask / PiecewiseLinearMask / "
                               "LinearTarget / constant target), Forcing(array) and MultipleForcings / tuples of them are supported")


def _node_table(grid, loc, D, fn, what):
    """fn(ξ) at the nodes of `loc` along D over the haloed index range (element ξ - 1 + H holds node ξ)"""
    d = _DIRS.index(D)
    if grid.topology[d] is Flat:
        raise ValueError(f"a {what} along {D}, which is Flat: the reference has no method for it (relaxation.jl Flat methods take the "
                         "remaining coordinates only)")
    F, Cn = ((grid.xᶠᵃᵃ, grid.xᶜᵃᵃ), (grid.yᵃᶠᵃ, grid.yᵃᶜᵃ), (grid.zᵃᵃᶠ, grid.zᵃᵃᶜ))[d]
    nodes = np.asarray(F if loc[d] is Face else Cn, dtype=np.float64)
    n = grid.total_size(loc)[d]
    if nodes.shape != (n,):
        raise ValueError(f"node array along {D} has {nodes.shape[0]} entries, the parent array {n}")
    return np.ascontiguousarray(fn(nodes), dtype=np.float64)


class Term:
    """one ocn_forcing_t: kind 1 (array), 2 (relaxation) with the host tables it points to, or 3 (function) with its recorded program
    and the model fields of its dependency slots"""

    def __init__(self, kind, array=None, mask_dir=-1, mask_table=None, rate_mask=0.0, target_dir=-1, target_table=None, target=0.0,
                 program=None, dep_names=()):
        self.kind, self.array = kind, array
        self.mask_dir, self.mask_table, self.rate_mask = mask_dir, mask_table, float(rate_mask)
        self.target_dir, self.target_table, self.target = target_dir, target_table, float(target)
        self.program, self.dep_names = program, tuple(dep_names)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _is_function(f):
    """a mask or target that is the user's own function: recorded, not tabulated"""
    return (callable(f) and not isinstance(f, type) and f is not onefunction and f is not zerofunction
            and not isinstance(f, (GaussianMask, PiecewiseLinearMask, LinearTarget)))


def _recorded_builtin(f, coordinate, what):
    """a built-in mask or target next to a function: its reference formula (relaxation.jl), recorded on the symbol of its coordinate"""
    from . import boundary_functions as bf
    if f.D not in coordinate:
        raise ValueError(f"a {what} along {f.D}, which is Flat: the reference has no method for it (relaxation.jl Flat methods take the "
                         "remaining coordinates only)")
    xi = coordinate[f.D]
    if isinstance(f, GaussianMask):
        return bf.exp(-(xi - f.center) ** 2 / (2 * (f.width * f.width)))
    if isinstance(f, PiecewiseLinearMask):
        return bf.max_(0.0, 1.0 - abs(xi - f.center) / f.width)
    return f.intercept + f.gradient * xi


def _function_relaxation_term(r, grid, loc, name):
    """Relaxation with a function mask or target: rate * mask(X...) * (target(X..., t) - φ) as the reference evaluates it
    (relaxation.jl:80-101), recorded once. X: the nodes of the forced field's location, Flat directions dropped; φ: dependency slot 0"""
    from .boundary_functions import trace
    dims = [d for d in range(3) if grid.topology[d] is not Flat]

    def known(f, what):
        if not (_is_function(f) or isinstance(f, (GaussianMask, PiecewiseLinearMask, LinearTarget))):
            raise _unsupported(f)
        return f

    def relaxation(*args):
        X, t, phi = args[:len(dims)], args[len(dims)], args[len(dims) + 1]
        coordinate = {_DIRS[d]: x for d, x in zip(dims, X)}
        if r.mask is onefunction:
            a = r.rate                                                  # rate * 1
        elif _is_function(r.mask):
            a = r.rate * r.mask(*X)
        else:
            a = r.rate * _recorded_builtin(known(r.mask, "mask"), coordinate, "mask")
        if r.target is zerofunction:
            b = 0.0                                                     # `0 - φ`
        elif _is_number(r.target):
            b = float(r.target)
        elif _is_function(r.target):
            b = r.target(*X, t)
        else:
            b = _recorded_builtin(known(r.target, "target"), coordinate, "target")
        return a * (b - phi)

    return Term(3, program=trace(relaxation, dims, 1), dep_names=(name,))


def _relaxation_term(r, grid, loc, name=None):
    if _is_function(r.mask) or _is_function(r.target):
        return _function_relaxation_term(r, grid, loc, name)
    if r.mask is onefunction:
        mask_dir, mask_table, rate_mask = -1, None, r.rate             # rate * 1
    elif isinstance(r.mask, (GaussianMask, PiecewiseLinearMask)):
        mask_dir = _DIRS.index(r.mask.D)
        # `f.rate * f.mask(x, y, z)`: the product per node, as the reference forms it per cell
        mask_table = _node_table(grid, loc, r.mask.D, lambda x: r.rate * r.mask(x), "mask")
        rate_mask = 0.0
    else:
        raise _unsupported(r.mask)
    if r.target is zerofunction:
        target_dir, target_table, target = -1, None, 0.0               # `0 - φ`
    elif isinstance(r.target, (int, float, np.integer, np.floating)) and not isinstance(r.target, bool):
        target_dir, target_table, target = -1, None, float(r.target)
    elif isinstance(r.target, LinearTarget):
        target_dir = _DIRS.index(r.target.D)
        target_table, target = _node_table(grid, loc, r.target.D, r.target, "target"), 0.0
    else:
        raise _unsupported(r.target)
    return Term(2, mask_dir=mask_dir, mask_table=mask_table, rate_mask=rate_mask, target_dir=target_dir, target_table=target_table,
                target=target)


def _array_term(a, grid):
    from .fields import Field
    if isinstance(a, Field):
        if tuple(a.loc) != (Center, Center, Center) or tuple(a.shape) != tuple(grid.total_size((Center, Center, Center))):
            raise ValueError(f"a Field forcing must be a (Center, Center, Center) field of the model's grid, got {a.loc} of shape {a.shape}")
        return Term(1, array=a)
    a = np.asarray(a)
    if a.shape != tuple(grid.size):
        raise ValueError(f"Forcing(array) needs an array of size(grid) = {tuple(grid.size)}, got {a.shape}")
    return Term(1, array=np.asarray(a, dtype=np.float64))


def regularize_forcing(f, grid, loc, name=None):
    """regularize_forcing (model_forcing.jl, multiple_forcings.jl): a forcing -> list of Terms, in summation order; `name`: the forced
    field, the dependency of a recorded relaxation"""
    from .fields import Field
    if isinstance(f, MultipleForcings):
        f = f.forcings
    if isinstance(f, (tuple, list)):
        terms = []
        for g in f:
            if isinstance(g, (tuple, list, MultipleForcings)):
                raise _unsupported(g)             # the reference sums a flat tuple; a nested one is not a forcing
            terms += regularize_forcing(g, grid, loc, name)
        return terms
    if isinstance(f, Relaxation):
        return [_relaxation_term(f, grid, loc, name)]
    if isinstance(f, ArrayForcing):
        return [_array_term(f.array, grid)]
    if isinstance(f, (np.ndarray, Field)):
        return [_array_term(f, grid)]
    raise _unsupported(f)


def model_forcing(grid, field_locations, forcing):
    """model_forcing(model_fields; forcings...) (model_forcing.jl): {name: [Term, ...]} for the named fields; `field_locations` maps every
    model field name to its location. An unknown name is refused."""
    out = {}
    for name, f in dict(forcing or {}).items():
        if name not in field_locations:
            raise NotImplementedError(f"forcing given for {name}, which is not a velocity or tracer of the model "
                                      f"({', '.join(field_locations)})")
        if f is None:
            continue
        terms = regularize_forcing(f, grid, field_locations[name], name)
        if len(terms) > _MAX_TERMS:
            raise ValueError(f"{len(terms)} forcing terms for {name}: at most {_MAX_TERMS}")
        out[name] = terms
    functions = sum(t.kind == 3 for terms in out.values() for t in terms)
    if functions > _MAX_FUNCTIONS:
        raise ValueError(f"{functions} function-valued forcing terms: the limit of a model is {_MAX_FUNCTIONS} function terms")
    return out


_MAX_TERMS = 8          # OCN_MAX_FORCING_TERMS
_MAX_FUNCTIONS = 16     # function terms of one model (ocn_forcing_function.h)


def refuse_functions_on_partitions(terms_by_field, grid):
    """function terms are served on one device. Raises NotImplementedError otherwise -- called before anything touches the device."""
    if hasattr(grid, "local") and any(t.kind == 3 for terms in terms_by_field.values() for t in terms):
        raise NotImplementedError("a Relaxation with a function mask or target is not served on partitioned grids")


def set_forcing(handle, field_index, terms, grid, keep, cname=None):
    """ocn_model_set_forcing for one field. Arrays become device buffers (numpy: owned, appended to `keep`; Field: borrowed). cname: model
    field name -> the library's ("u", "v", "w", "c0" ..), for the dependencies of function terms"""
    from .fields import CenterField
    arr = (_lib.Forcing * max(1, len(terms)))()
    host = []
    for q, t in enumerate(terms):
        e = arr[q]
        e.kind = t.kind
        if t.kind == 1:
            fld = t.array
            if isinstance(fld, np.ndarray):
                dev = CenterField(grid)
                dev.set(fld)
                keep.append(dev)
                fld = dev
            else:
                keep.append(fld)
            e.array = fld.data
        if t.kind == 3:
            from .boundary_functions import program_array
            program, e.n = program_array(t.program)
            names = (C.c_char_p * max(len(t.dep_names), 1))(*[(cname(d) if cname else d).encode() for d in t.dep_names])
            host += [program, names]
            e.program, e.dep_names, e.ndeps = C.cast(program, C.c_void_p), C.cast(names, C.c_void_p), len(t.dep_names)
        e.mask_dir, e.rate_mask, e.target_dir, e.target = t.mask_dir, t.rate_mask, t.target_dir, t.target
        if t.mask_table is not None:
            host.append(t.mask_table)
            e.mask_table = t.mask_table.ctypes.data_as(C.POINTER(C.c_double))
        if t.target_table is not None:
            host.append(t.target_table)
            e.target_table = t.target_table.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.lib().ocn_model_set_forcing(handle, int(field_index), arr, len(terms)))


def node_coordinates(grid, loc):
    """the node coordinates over the interior of `loc`, shaped to broadcast as (x, y, z); None along a Flat direction"""
    n, H = grid.interior_size(loc), grid.halo_size
    nodes = ((grid.xᶠᵃᵃ, grid.xᶜᵃᵃ), (grid.yᵃᶠᵃ, grid.yᵃᶜᵃ), (grid.zᵃᵃᶠ, grid.zᵃᵃᶜ))
    out = []
    for d in range(3):
        if grid.topology[d] is Flat:
            out.append(None)
            continue
        shape = [1, 1, 1]
        shape[d] = n[d]
        out.append(np.asarray(nodes[d][0] if loc[d] is Face else nodes[d][1], dtype=np.float64)[H[d]:H[d] + n[d]].reshape(shape))
    return out


def evaluate(terms, grid, loc, phi, t=0.0):
    """host twin of ocn_forcing.h's forcing_sum over the interior of `loc` (tests): φ is the field's interior array, t the clock's time.
    A function term is interpreted with numpy; its one dependency is φ (a recorded relaxation)"""
    from .fields import Field
    nx, ny, nz = grid.interior_size(loc)
    H = grid.halo_size

    time = t

    def tab(t, d):
        sl = slice(H[d], H[d] + (nx, ny, nz)[d])
        shape = [1, 1, 1]
        shape[d] = (nx, ny, nz)[d]
        return t[sl].reshape(shape)

    def one(t):
        if t.kind == 1:
            a = t.array.interior() if isinstance(t.array, Field) else np.asarray(t.array, dtype=np.float64)
            out = np.zeros((nx, ny, nz))
            mx, my, mz = min(nx, a.shape[0]), min(ny, a.shape[1]), min(nz, a.shape[2])
            out[:mx, :my, :mz] = a[:mx, :my, :mz]
            return out
        if t.kind == 3:
            from .boundary_functions import interpret
            return np.array(np.broadcast_to(interpret(t.program, node_coordinates(grid, loc), time, [phi] * len(t.dep_names)), (nx, ny, nz)))
        a = t.rate_mask if t.mask_dir < 0 else tab(t.mask_table, t.mask_dir)
        b = t.target if t.target_dir < 0 else tab(t.target_table, t.target_dir)
        return a * (b - phi)

    if len(terms) > 4:
        total = np.zeros((nx, ny, nz))
        for t in terms:
            total = total + one(t)
        return total
    s = one(terms[0])
    for t in terms[1:]:
        s = s + one(t)
    return s


__all__ = ["Relaxation", "GaussianMask", "PiecewiseLinearMask", "LinearTarget", "MultipleForcings", "Forcing", "ContinuousForcing",
           "DiscreteForcing", "AdvectiveForcing", "onefunction", "zerofunction", "model_forcing"]
