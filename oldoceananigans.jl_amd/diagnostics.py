"""On-device diagnostics (reference: src/AbstractOperations/binary_operations.jl, computed_field.jl, metric_field_reductions.jl,
src/Fields/scans.jl, src/Fields/field.jl:673-816).

    wu = ocn.Field(ocn.Average(w * u, dims=(1, 2)))      # computed on construction
    ocn.compute(wu); wu.interior()                       # a (1, 1, Nz + 1) host array

A BinaryOperation (`a + b`, `a - b`, `a * b`, `a / b`, `a ** 2` of a Field and a Field or a number) and the scans (Average, Integral,
CumulativeIntegral, Reduction, Accumulation) are descriptors: no device work happens until `Field(operand)` / `compute(field)`, which run
the kernels of csrc/ocn_diagnostics.h on the library's stream, after whatever step came before.

Two evaluators serve them. ONE operation node over fields and numbers keeps the fixed one (ocn_operand_t). Everything deeper is a
stencil program (operators.py): KernelFunctionOperation(location, kernel_function, grid, *arguments) records a kernel function written
with the operators of ocn.operators; Derivative (ocn.dx / dy / dz), UnaryOperation (ocn.sqrt .. tanh of a field, abs(f), -f), ocn.at and a
BinaryOperation with such operands are lowered to the same programs as the reference's getindex evaluates them
(AbstractOperations/derivatives.jl:23, unary_operations.jl:21, binary_operations.jl:25).

Refused by name (NotImplementedError, before any device call): condition= / mask=, arithmetic on a BinaryOperation (materialise it with
Field(op) first, or write a KernelFunctionOperation), functions, strings and arrays as operands, reduced fields as operands, partitioned
grids; fields of different grids are a ValueError."""
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
    if hasattr(grid, "immersed_boundary"):
        # the reference's reductions and operations on an immersed grid exclude the immersed cells through a condition
        # (immersed_reductions.jl), which this library does not have
        from .immersed_boundaries import refuse
        refuse("a diagnostic (operation, reduction, scan or time average; the reference excludes immersed cells through a condition)")
    if any(t in (FullyConnected, RightConnected, LeftConnected) for t in grid.topology):
        raise NotImplementedError("diagnostics on a partitioned grid are not built: gather the fields of the ranks (or reduce per rank and "
                                  "combine on the host)")


def _check_field(f):
    if not isinstance(f, Field):
        raise NotImplementedError(f"{type(f).__name__} as an operand: a Field, a Derivative, a UnaryOperation, a KernelFunctionOperation or one "
                                  "BinaryOperation of those and numbers is served; functions, strings and arrays are not")
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

    def __init__(self, op, a, b, location=None):
        fields = [x for x in (a, b) if not isinstance(x, numbers.Real)]
        for x in fields:
            if isinstance(x, (BinaryOperation, Scan, KernelFunctionOperation)):
                raise NotImplementedError("nested operations are not built: materialise the inner one first with Field(op) and use that "
                                          "field as the operand (KernelFunctionOperation is the route for deeper expressions)")
            if not isinstance(x, (Derivative, UnaryOperation)):
                _check_field(x)
        if not fields:
            raise TypeError("an operation needs a Field operand")
        if len(fields) == 2 and fields[0].grid is not fields[1].grid:
            raise ValueError("the operands live on different grids")          # validate_grid (AbstractOperations/AbstractOperations.jl)
        self.op, self.a, self.b = op, a, b
        self.grid = fields[0].grid
        self.location = _location(fields[0]) if location is None else _as_location(location)
        self.interp_a = "identity" if isinstance(a, numbers.Real) else interpolation_operator(_location(a), self.location)
        self.interp_b = "identity" if isinstance(b, numbers.Real) else interpolation_operator(_location(b), self.location)

    @property
    def fixed(self):
        """whether the fixed evaluator (ocn_operand_t) serves this node: fields and numbers at the first field's location"""
        operands = [x for x in (self.a, self.b) if not isinstance(x, numbers.Real)]
        return all(isinstance(x, Field) for x in operands) and self.location == operands[0].loc

    def _nested(self, *_):
        raise NotImplementedError("nested operations are not built: materialise this one first with Field(op) and use that field as the operand "
                                  "(KernelFunctionOperation is the route for deeper expressions)")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __pow__ = _nested

    def __repr__(self):
        loc = ", ".join(l.__name__ for l in self.location)
        return f"BinaryOperation at ({loc}): {self.op}"


def binary_operation(op, a, b):
    for x in (a, b):
        if isinstance(x, bool) or not isinstance(x, (numbers.Real, Field, BinaryOperation, Scan, Derivative, UnaryOperation, KernelFunctionOperation)):
            raise NotImplementedError(f"{type(x).__name__} as an operand: a Field or a number is served")
    return BinaryOperation(op, a, b)


def power(a, exponent):
    """a ** 2 is a * a; other exponents are refused"""
    if isinstance(exponent, bool) or not isinstance(exponent, numbers.Real) or exponent != 2:
        raise NotImplementedError(f"a ** {exponent!r}: only the exponent 2 is built (as a * a)")
    return BinaryOperation("*", a, a)


# ---------------------------------------------------------------------------------------------------------------------
# nodes that are lowered to stencil programs (operators.py)
# ---------------------------------------------------------------------------------------------------------------------
def _as_location(loc):
    loc = tuple(l if isinstance(l, type) else type(l) for l in loc)
    if len(loc) != 3 or any(l not in (Center, Face) for l in loc):
        raise ValueError(f"location {loc!r}: a 3-tuple of Center / Face")
    return loc


def _location(x):
    return x.loc if isinstance(x, Field) else x.location


def _flip(l):
    """flip (derivatives.jl:42-43)"""
    return Face if l is Center else Center


class _Node:
    """what the tree nodes below share: arithmetic that builds a BinaryOperation / UnaryOperation, and the cached lowering"""

    __array_ufunc__ = None

    def __add__(self, o): return binary_operation("+", self, o)
    def __radd__(self, o): return binary_operation("+", o, self)
    def __sub__(self, o): return binary_operation("-", self, o)
    def __rsub__(self, o): return binary_operation("-", o, self)
    def __mul__(self, o): return binary_operation("*", self, o)
    def __rmul__(self, o): return binary_operation("*", o, self)
    def __truediv__(self, o): return binary_operation("/", self, o)
    def __rtruediv__(self, o): return binary_operation("/", o, self)
    def __pow__(self, e): return power(self, e)
    def __neg__(self): return UnaryOperation("neg", self)
    def __abs__(self): return UnaryOperation("abs", self)


def _check_argument(arg, what):
    if isinstance(arg, (Scan, KernelFunctionOperation)):
        raise NotImplementedError(f"{type(arg).__name__} as the argument of a {what}: materialise it first with Field(...)")
    if not isinstance(arg, (Derivative, UnaryOperation, BinaryOperation)):
        _check_field(arg)
    _check_grid(arg.grid)
    return arg


class Derivative(_Node):
    """Derivative{LX, LY, LZ}(∂, arg, ▶, grid) (derivatives.jl:3-34): ∂ along `direction` (0, 1, 2) of `arg` where it lands -- arg's location
    with the direction flipped -- then interpolated to `location` by the operator `interp` names; getindex is ▶(i, j, k, grid, ∂, arg) (:23)"""

    def __init__(self, direction, arg, location=None):
        self.direction, self.arg = int(direction), _check_argument(arg, "Derivative")
        self.grid = arg.grid
        La = _location(arg)
        self.derivative_location = tuple(_flip(l) if d == self.direction else l for d, l in enumerate(La))
        self.location = self.derivative_location if location is None else _as_location(location)
        # ∂x(LX, LY, LZ) (derivatives.jl:48-54): the operator named for where the derivative lands
        self.operator = "d" + "xyz"[self.direction] + "".join(_SUP[l] for l in self.derivative_location)
        self.interp = interpolation_operator(self.derivative_location, self.location)

    def __repr__(self):
        return f"Derivative at ({', '.join(l.__name__ for l in self.location)}): ∂{'xyz'[self.direction]} via {self.interp}"


UNARY_OPERATORS = ("identity", "neg", "abs", "sqrt", "exp", "log", "sin", "cos", "tanh")


class UnaryOperation(_Node):
    """UnaryOperation{LX, LY, LZ}(op, arg, ▶, grid) (unary_operations.jl:3-34): op at arg's location, then interpolated to `location`;
    getindex is ▶(i, j, k, grid, op, arg) (:21). op: one of UNARY_OPERATORS ("identity" is at.jl's interpolate_identity, :28-37)"""

    def __init__(self, op, arg, location=None):
        if op in ("log10", "tan", "sinh", "cosh"):
            raise NotImplementedError(f"{op}(field): the reference's {op} has no instruction in a stencil program")
        if op not in UNARY_OPERATORS:
            raise NotImplementedError(f"{op}(field): the unary operations with an instruction are {', '.join(UNARY_OPERATORS[1:])}")
        self.op, self.arg = op, _check_argument(arg, "UnaryOperation")
        self.grid = arg.grid
        self.location = _location(arg) if location is None else _as_location(location)
        self.interp = interpolation_operator(_location(arg), self.location)

    def __repr__(self):
        return f"UnaryOperation at ({', '.join(l.__name__ for l in self.location)}): {self.op} via {self.interp}"


class KernelFunctionOperation:
    """KernelFunctionOperation{LX, LY, LZ}(kernel_function, grid, arguments...) (kernel_function_operation.jl:58-70) as
    KernelFunctionOperation(location, kernel_function, grid, *arguments). The function is called ONCE, here, as
    kernel_function(i, j, k, grid, *arguments) with index symbols and, for every Field among the arguments, a field symbol
    (operators.record); anything else is handed over untouched. ValueError: a limit, or the reach rule -- an offset the grid's halo does
    not cover; TypeError: a misused symbol."""

    def __init__(self, location, kernel_function, grid, *arguments):
        from . import operators
        if not callable(kernel_function):
            raise TypeError("kernel_function must be callable")
        self.location = _as_location(location)
        _check_grid(grid)
        for a in arguments:
            if isinstance(a, Field):
                _check_field(a)
                if a.grid is not grid:
                    raise ValueError("the operands live on different grids")
            elif isinstance(a, _NODES + (Scan,)):
                raise NotImplementedError(f"{type(a).__name__} as an argument of a KernelFunctionOperation: materialise it first with Field(...)")
        self.kernel_function, self.grid, self.arguments = kernel_function, grid, tuple(arguments)
        self.stencil = operators.record(kernel_function, grid, self.location, self.arguments)

    __array_ufunc__ = None

    def _nested(self, *_):
        raise NotImplementedError("arithmetic on a KernelFunctionOperation is not built: write it inside the kernel function, or materialise "
                                  "this one first with Field(op)")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __pow__ = _nested

    def __repr__(self):
        # Base.show (kernel_function_operation.jl:83-96)
        loc = ", ".join(l.__name__ for l in self.location)
        args = "()" if not self.arguments else "(" + ", ".join('"Field"' if isinstance(a, Field) else repr(a) for a in self.arguments) + ")"
        return (f"KernelFunctionOperation at ({loc})\n├── grid: {self.grid!r}\n"
                f"├── kernel_function: {getattr(self.kernel_function, '__name__', repr(self.kernel_function))}\n└── arguments: {args}")


_NODES = (BinaryOperation, Derivative, UnaryOperation, KernelFunctionOperation)


def _derivative(direction):
    def d(*args):
        if len(args) == 1:
            return Derivative(direction, args[0])
        if len(args) == 2:
            return Derivative(direction, args[1], args[0])
        raise TypeError(f"d{'xyz'[direction]}(f) or d{'xyz'[direction]}(location, f)")
    d.__name__ = "d" + "xyz"[direction]
    d.__doc__ = (f"∂{'xyz'[direction]}(arg) / ∂{'xyz'[direction]}(L, arg) (derivatives.jl:65-107): the derivative of a Field or an operation, by "
                 "default where it lands (arg's location with the direction flipped), else interpolated to L")
    return d


dx, dy, dz = _derivative(0), _derivative(1), _derivative(2)


def unary_operation(op, arg):
    """what ocn.sqrt .. ocn.tanh answer for a Field or an operation"""
    return UnaryOperation(op, arg)


def at(location, node):
    """@at location node (at.jl:45-55) through the reference's at(loc, ·) methods: a BinaryOperation is rebuilt at `location` with both
    operands relocated (binary_operations.jl:32), a UnaryOperation likewise (unary_operations.jl:37), a Derivative is taken where it lands
    and interpolated to `location` with its argument as it is (derivatives.jl:39); a Field elsewhere is interpolated
    (interpolate_identity, at.jl:28-37), a Field at `location` and a number stay"""
    location = _as_location(location)
    relocated = _at(location, node)
    if isinstance(relocated, Field) and relocated.loc != location:
        return UnaryOperation("identity", relocated, location)
    return relocated


def _at(location, node):
    if isinstance(node, BinaryOperation):
        return BinaryOperation(node.op, _at(location, node.a), _at(location, node.b), location)
    if isinstance(node, UnaryOperation):
        return UnaryOperation(node.op, _at(location, node.arg), location)
    if isinstance(node, Derivative):
        return Derivative(node.direction, node.arg, location)
    if isinstance(node, (Field, numbers.Real)):
        return node                                            # at(loc, f) = f (AbstractOperations.jl:48)
    raise NotImplementedError(f"at(location, {type(node).__name__}): a Field or a tree of BinaryOperation, UnaryOperation and Derivative")


def lower(node):
    """the StencilProgram of a Field, a BinaryOperation, a Derivative, a UnaryOperation or a KernelFunctionOperation (cached on the node):
    the tree is evaluated once with symbols, each node as the reference's getindex evaluates it"""
    from . import boundary_functions as bf
    from . import operators
    if isinstance(node, KernelFunctionOperation):
        return node.stencil
    cached = None if isinstance(node, Field) else getattr(node, "_stencil", None)
    if cached is not None:
        return cached
    fields = []

    def collect(x):
        if isinstance(x, Field):
            if not any(x is f for f in fields):
                fields.append(x)
        elif isinstance(x, BinaryOperation):
            collect(x.a), collect(x.b)
        elif isinstance(x, (Derivative, UnaryOperation)):
            collect(x.arg)
    collect(node)
    if any(f.grid is not fields[0].grid for f in fields):
        raise ValueError("the operands live on different grids")
    unary = {"identity": lambda x: x, "neg": lambda x: -x, "abs": abs, "sqrt": bf.sqrt, "exp": bf.exp, "log": bf.log, "sin": bf.sin,
             "cos": bf.cos, "tanh": bf.tanh}
    binary = {"+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": lambda x, y: x / y}

    def kernel_function(i, j, k, grid, *symbols):
        def operand(x):
            """what an operator takes: a field symbol, a number, or the function that evaluates the node"""
            if isinstance(x, Field):
                return symbols[next(q for q, f in enumerate(fields) if f is x)]
            if isinstance(x, numbers.Real):
                return float(x)
            return lambda i, j, k, grid: evaluate(x, i, j, k)

        def evaluate(x, i, j, k):
            if isinstance(x, BinaryOperation):
                a = operators.interpolation(x.interp_a)(i, j, k, grid, operand(x.a))
                b = operators.interpolation(x.interp_b)(i, j, k, grid, operand(x.b))
                return binary[x.op](a, b)
            if isinstance(x, Derivative):
                return operators.interpolation(x.interp)(i, j, k, grid, getattr(operators, x.operator), operand(x.arg))
            op = unary[x.op]
            return operators.interpolation(x.interp)(i, j, k, grid, lambda i, j, k, grid, a: op(operators.identity(i, j, k, grid, a)), operand(x.arg))
        return operators.identity(i, j, k, grid, operand(node))

    stencil = operators.record(kernel_function, node.grid, _location(node), fields)
    if not isinstance(node, Field):
        node._stencil = stencil
    return stencil


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
    if not isinstance(operand, _NODES):
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
        operand_location = _location(operand)
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
    if isinstance(x, _NODES + (Scan,)):
        _check_grid(x.grid)
        return x
    raise TypeError(f"Field({type(x).__name__}): a location tuple, an operation (BinaryOperation, Derivative, UnaryOperation, "
                    "KernelFunctionOperation) or a scan")


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
    inner = operand.operand if isinstance(operand, Scan) else operand
    stencil = not (isinstance(inner, Field) or (isinstance(inner, BinaryOperation) and inner.fixed))      # which evaluator
    if not isinstance(operand, Scan):
        (kernels.compute_stencil if stencil else kernels.compute_operation)(grid, operand, field)
        fill_halo_regions(field)
    elif operand.reducing:
        (kernels.reduce_stencil if stencil else kernels.reduce_operation)(grid, inner, operand.kind, operand.dims, operand.use_metric,
                                                                           operand.absolute, field)
    else:
        (kernels.accumulate_stencil if stencil else kernels.accumulate_operation)(grid, inner, operand.dims[0], operand.reverse,
                                                                                   operand.use_metric, field)
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
