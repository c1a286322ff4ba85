"""On-device diagnostics (reference: src/AbstractOperations/binary_operations.jl, computed_field.jl, metric_field_reductions.jl,
src/Fields/scans.jl, src/Fields/field.jl:673-816).

    wu = ocn.Field(ocn.Average(w * u, dims=(1, 2)))      # computed on construction
    ocn.compute(wu); wu.interior()                       # a (1, 1, Nz + 1) host array

A BinaryOperation (`a + b`, `a - b`, `a * b`, `a / b`, `a ** 2` of a Field and a Field or a number) and the scans (Average, Integral,
CumulativeIntegral, Reduction, Accumulation) are descriptors: no device work happens until `Field(operand)` / `compute(field)`, which run
the kernels of csrc/ocn_diagnostics.h on the library's stream, after whatever step came before.

Served: ONE operation node over fields of one grid. Refused by name (NotImplementedError, before any device call): condition= / mask=,
derivative and unary operands, nested operations (materialise the inner one with Field(op) first), reduced fields as operands,
partitioned grids; fields of different grids are a ValueError."""
import numbers

from . import _lib
from .fields import Field, fill_halo_regions
from .grids import Center, Face, FullyConnected, LeftConnected, RightConnected

_OP_CODE = {"identity": 0, "+": 1, "-": 2, "*": 3, "/": 4}
_KIND_CODE = {"sum": 0, "maximum": 1, "minimum": 2, "average": 3}
_LOC = {Center: 0, Face: 1}
_SUP = {Center: "ᶜ", Face: "ᶠ"}


class FieldStatus:
    """FieldStatus (Fields/field.jl): the time a computed field was last computed at (compute_at)"""

    def __init__(self):
        self.time = 0.0


def _check_grid(grid):
    if any(t in (FullyConnected, RightConnected, LeftConnected) for t in grid.topology):
        raise NotImplementedError("diagnostics on a partitioned grid are not built: gather the fields of the ranks (or reduce per rank and "
                                  "combine on the host)")


def _check_field(f):
    if not isinstance(f, Field):
        raise NotImplementedError(f"{type(f).__name__} as an operand: a Field or one BinaryOperation of Fields and numbers is served; "
                                  "derivatives, unary operations and functions are not built")
    if any(l is None for l in f.loc):
        raise NotImplementedError("a reduced field as an operand is not built")
    _check_grid(f.grid)


def interpolation_operator(from_loc, to_loc):
    """the NAME of interpolation_operator(from, to) (Operators/interpolation_utils.jl:55-69), e.g. "ℑxzᶜᵃᶠ"; "identity" where nothing moves"""
    codes = ["ᵃ" if a is b else _SUP[b] for a, b in zip(from_loc, to_loc)]
    if all(c == "ᵃ" for c in codes):
        return "identity"
    return "ℑ" + "".join(d for d, c in zip("xyz", codes) if c != "ᵃ") + "".join(codes)


class BinaryOperation:
    """op(▶a(a), ▶b(b)) at `location` (binary_operations.jl:5-25): the location of the first field operand (:109-135), the other field
    interpolated to it by the operator `interp_a` / `interp_b` names (:38-43)"""

    def __init__(self, op, a, b):
        fields = [x for x in (a, b) if not isinstance(x, numbers.Real)]
        for x in fields:
            if isinstance(x, (BinaryOperation, Scan)):
                raise NotImplementedError("nested operations are not built: materialise the inner one first with Field(op) and use that "
                                          "field as the operand")
            _check_field(x)
        if not fields:
            raise TypeError("an operation needs a Field operand")
        if len(fields) == 2 and fields[0].grid is not fields[1].grid:
            raise ValueError("the operands live on different grids")          # validate_grid (AbstractOperations/AbstractOperations.jl)
        self.op, self.a, self.b = op, a, b
        self.grid = fields[0].grid
        self.location = fields[0].loc
        self.interp_a = interpolation_operator(a.loc, self.location) if isinstance(a, Field) else "identity"
        self.interp_b = interpolation_operator(b.loc, self.location) if isinstance(b, Field) else "identity"

    def _nested(self, *_):
        raise NotImplementedError("nested operations are not built: materialise this one first with Field(op) and use that field as the operand")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __pow__ = _nested

    def __repr__(self):
        loc = ", ".join(l.__name__ for l in self.location)
        return f"BinaryOperation at ({loc}): {self.op}"


def binary_operation(op, a, b):
    for x in (a, b):
        if isinstance(x, bool) or not isinstance(x, (numbers.Real, Field, BinaryOperation, Scan)):
            raise NotImplementedError(f"{type(x).__name__} as an operand: a Field or a number is served")
    return BinaryOperation(op, a, b)


def power(a, exponent):
    """a ** 2 is a * a; other exponents are refused"""
    if isinstance(exponent, bool) or not isinstance(exponent, numbers.Real) or exponent != 2:
        raise NotImplementedError(f"a ** {exponent!r}: only the exponent 2 is built (as a * a)")
    return BinaryOperation("*", a, a)


def _filter_dims(dims):
    """tupleit + the 1-based directions of the reference; None is Colon: (1, 2, 3)"""
    if dims is None:
        return (1, 2, 3)
    dims = (dims,) if isinstance(dims, numbers.Integral) else tuple(dims)
    if not dims or any(isinstance(d, bool) or not isinstance(d, numbers.Integral) or d not in (1, 2, 3) for d in dims) or len(set(dims)) != len(dims):
        raise ValueError(f"dims = {dims!r}: one or more of 1, 2, 3")
    return tuple(sorted(int(d) for d in dims))


def _refuse_conditions(kw):
    for name in ("condition", "mask"):
        if name in kw:
            raise NotImplementedError(f"{name}=: conditional operands (ConditionalOperation) are not built")
    if kw:
        raise TypeError(f"unexpected keyword {sorted(kw)[0]!r}")


def _check_operand(operand):
    if isinstance(operand, Scan):
        raise NotImplementedError("nested operations are not built: materialise the inner scan first with Field(scan)")
    if not isinstance(operand, BinaryOperation):
        _check_field(operand)
    return operand


def reduced_location(loc, dims):
    """reduced_location (Fields/field.jl:673-687)"""
    return tuple(None if d + 1 in dims else l for d, l in enumerate(loc))


class Scan:
    """Scan (Fields/scans.jl:18-23): what a scanned computed field is computed from"""

    reducing = True

    def __init__(self, kind, operand, dims, use_metric=False, absolute=False, reverse=False):
        self.kind, self.operand, self.dims = kind, _check_operand(operand), dims
        self.use_metric, self.absolute, self.reverse = bool(use_metric), bool(absolute), bool(reverse)
        self.grid = operand.grid
        operand_location = operand.location if isinstance(operand, BinaryOperation) else operand.loc
        self.location = reduced_location(operand_location, dims) if self.reducing else tuple(operand_location)

    def __repr__(self):
        return f"{type(self).__name__} {self.kind} over dims {self.dims}"


class Reduction(Scan):
    """Reduction(kind, operand, dims) with kind "sum" | "maximum" | "minimum" (Reduction(sum!, operand; dims), scans.jl:148)"""

    def __init__(self, kind, operand, dims, f=None, **kw):
        _refuse_conditions(kw)
        if kind not in ("sum", "maximum", "minimum"):
            raise NotImplementedError(f"Reduction({kind!r}, ...): sum, maximum and minimum are built")
        if f is not None and f is not abs:
            raise NotImplementedError("f: None or abs")
        if f is abs and kind == "sum":
            raise NotImplementedError("sum(abs, ...) is not built")
        super().__init__(kind, operand, _filter_dims(dims), absolute=f is abs)


class Average(Scan):
    """Average(operand, dims=None) (metric_field_reductions.jl:65-94): over regular directions the sum divided by the number of points;
    where a reduced direction is the stretched z the summand is operand * metric and the divisor the sum of the metric"""

    def __init__(self, operand, dims=None, **kw):
        _refuse_conditions(kw)
        dims = _filter_dims(dims)
        stretched = 3 in dims and not _check_operand(operand).grid.z_regular
        super().__init__("average", operand, dims, use_metric=stretched)


class Integral(Scan):
    """Integral(operand, dims=None) (metric_field_reductions.jl:144-150): the sum of operand * metric"""

    def __init__(self, operand, dims=None, **kw):
        _refuse_conditions(kw)
        super().__init__("sum", operand, _filter_dims(dims), use_metric=True)


class _Accumulating(Scan):
    reducing = False

    def __init__(self, operand, dims, reverse, use_metric):
        if isinstance(dims, bool) or not isinstance(dims, numbers.Integral) or dims not in (1, 2, 3):
            raise ValueError(f"{type(self).__name__} only supports dims=1, 2, or 3.")
        super().__init__("cumsum", operand, (int(dims),), use_metric=use_metric, reverse=reverse)


class CumulativeIntegral(_Accumulating):
    """CumulativeIntegral(operand, dims, reverse=False) (metric_field_reductions.jl:206-212): cumsum of operand * Δ of the direction"""

    def __init__(self, operand, dims, reverse=False, **kw):
        _refuse_conditions(kw)
        super().__init__(operand, dims, reverse, True)


class Accumulation(_Accumulating):
    """Accumulation("cumsum", operand, dims) (Accumulation(cumsum!, operand; dims), scans.jl:199)"""

    def __init__(self, kind, operand, dims, reverse=False, **kw):
        _refuse_conditions(kw)
        if kind != "cumsum":
            raise NotImplementedError(f"Accumulation({kind!r}, ...): cumsum is built")
        super().__init__(operand, dims, reverse, False)


def as_field_operand(x):
    """what Field(x) may be computed from"""
    if isinstance(x, (BinaryOperation, Scan)):
        _check_grid(x.grid)
        return x
    raise TypeError(f"Field({type(x).__name__}): a location tuple, a BinaryOperation or a scan")


# ---------------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------------
def operand_struct(operand):
    """the ocn_operand_t of a Field or a BinaryOperation (keeps nothing alive: pass it while the fields exist)"""
    s = _lib.Operand()
    if isinstance(operand, Field):
        s.op, s.a = 0, operand.data
        codes = [_LOC[l] for l in operand.loc]
        s.loc_a[:], s.loc[:] = codes, codes
        return s
    s.op = _OP_CODE[operand.op]
    for side, x in (("a", operand.a), ("b", operand.b)):
        if isinstance(x, Field):
            setattr(s, side, x.data)
            getattr(s, "loc_" + side)[:] = [_LOC[l] for l in x.loc]
        else:
            setattr(s, "c" + side, float(x))
    s.loc[:] = [_LOC[l] for l in operand.location]
    return s


def dims_mask(dims):
    mask = 0
    for d in dims:
        mask |= 1 << (d - 1)
    return mask


def compute(field):
    """compute!(field) (computed_field.jl:80-90, scans.jl:76-87): evaluate field.operand into field; a computed field of an operation
    then has its halos filled with the default conditions. Computed operands are NOT recomputed first: compute them in order. The
    operand's fields are read through their device pointers: a computed field of a model's fields (views that do not keep the model
    alive) must not be computed after the model is gone."""
    from . import kernels
    operand = getattr(field, "operand", None)
    if operand is None:
        return field                                           # compute!(field) of a plain field is a no-op (field.jl)
    grid = field.grid
    if isinstance(operand, BinaryOperation):
        kernels.compute_operation(grid, operand, field)
        fill_halo_regions(field)
    elif operand.reducing:
        kernels.reduce_operation(grid, operand.operand, operand.kind, operand.dims, operand.use_metric, operand.absolute, field)
    else:
        kernels.accumulate_operation(grid, operand.operand, operand.dims[0], operand.reverse, operand.use_metric, field)
    return field


def compute_at(field, time):
    """compute_at!(field, time) (Fields/field.jl): compute only when `time` differs from field.status.time, and record it"""
    status = getattr(field, "status", None)
    if status is None or time is None:
        return compute(field)
    if time != status.time:
        compute(field)
        status.time = time
    return field


# ---------------------------------------------------------------------------------------------------------------------
# allocating reductions (Fields/field.jl:735-816): a float for all dims, a reduced field otherwise. Not re-exported at top level: they
# would shadow builtins under `import *`.
# ---------------------------------------------------------------------------------------------------------------------
def _allocating(scan, dims):
    out = Field(scan)
    return float(out.interior()[0, 0, 0]) if dims is None else out


def sum(field, dims=None, **kw):                                # noqa: A001
    _refuse_conditions(kw)
    return _allocating(Reduction("sum", field, dims), dims)


def maximum(field, dims=None, f=None, **kw):
    _refuse_conditions(kw)
    return _allocating(Reduction("maximum", field, dims, f=f), dims)


def minimum(field, dims=None, f=None, **kw):
    _refuse_conditions(kw)
    return _allocating(Reduction("minimum", field, dims, f=f), dims)


def mean(field, dims=None, **kw):
    """mean(field; dims) (Statistics._mean, field.jl:798-813): sum / count -- never the metrics"""
    _refuse_conditions(kw)
    return _allocating(Scan("average", field, _filter_dims(dims)), dims)
