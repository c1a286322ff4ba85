"""Boundary functions: FluxBoundaryCondition(func, field_dependencies=..., parameters=...) (reference: src/BoundaryConditions/
continuous_boundary_function.jl:22-154, src/Utils/user_function_arguments.jl:22-39).

    drag_u = lambda x, y, t, u, v, p: -p.cD * ocn.sqrt(u ** 2 + v ** 2) * u
    u_bcs = ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=p))

A closure cannot cross the C ABI; a program can. When the model is built the function is called ONCE, on the host, with symbols for the
coordinates, the time and the dependencies. Every operation on a symbol records one instruction (ocn_expr_ins_t, include/ocn_mi355x.h), in
the order Python evaluates them: no simplification, no reassociation. One small kernel then evaluates the list at every boundary point,
with the fields and the clock of that moment, into the array of an ordinary array-valued Flux condition.

What a function may do with its arguments: + - * /, unary minus, abs, ** (x ** 2 and x ** 3 are repeated multiplication, like Julia's
literal_pow), the comparisons < <= > >=, and ocn.sqrt / exp / log / sin / cos / tanh / ifelse / min_ / max_ (the builtins min and max
ask a symbol for its truth value and cannot be recorded). Python numbers and parameter values become constants; an operation on two
numbers is done by Python. Control flow on a symbol (`if u > 0:`) is a TypeError: write ocn.ifelse(u > 0, a, b)."""
import numbers

import numpy as np

from .grids import Center, Face, Flat

MAX_INSTRUCTIONS = 64
MAX_DEPENDENCIES = 8

# OCN_EXPR_* (include/ocn_mi355x.h)
OPS = {"const": 0, "coord": 1, "time": 2, "field": 3, "+": 4, "-": 5, "*": 6, "/": 7, "neg": 8, "abs": 9, "min": 10, "max": 11, "sqrt": 12,
       "exp": 13, "log": 14, "sin": 15, "cos": 16, "tanh": 17, "pow": 18, "<": 19, "<=": 20, ">": 21, ">=": 22, "select": 23}
OP_NAMES = {v: k for k, v in OPS.items()}


class _Trace:
    """the instructions recorded so far: tuples (op, a, b, c, imm)"""

    def __init__(self):
        self.instructions = []

    def emit(self, op, a=0, b=0, c=0, imm=0.0):
        if len(self.instructions) == MAX_INSTRUCTIONS:
            raise ValueError(f"the function performs more than {MAX_INSTRUCTIONS} operations: the limit of a traced function is "
                             f"{MAX_INSTRUCTIONS} instructions")
        self.instructions.append((OPS[op], int(a), int(b), int(c), float(imm)))
        return len(self.instructions) - 1

    def value(self, x):
        """the index of the value of x: a symbol's own (a leaf is emitted on first use), or a new constant"""
        if isinstance(x, Symbol):
            if x.trace is not self:
                raise ValueError("a symbol of another function")
            if x.index is None:
                x.index = self.emit(*x.leaf)
            return x.index
        if isinstance(x, (bool, np.bool_)):
            x = 1.0 if x else 0.0
        if not isinstance(x, (numbers.Real, np.floating, np.integer)):
            raise TypeError(f"{type(x).__name__} in a function: symbols and real numbers can be recorded")
        return self.emit("const", imm=float(x))


class Symbol:
    """a value of the traced function: a coordinate, the time, a dependency (leaves, emitted when first used) or the result of an operation"""

    __array_ufunc__ = None    # a numpy scalar on the left of an operation defers to the reflected method
    __hash__ = object.__hash__

    def __init__(self, trace, index=None, leaf=None):
        self.trace, self.index, self.leaf = trace, index, leaf

    def _op(self, op, *operands):
        idx = [self.trace.value(x) for x in operands]
        return Symbol(self.trace, self.trace.emit(op, *idx))

    def __add__(self, o): return self._op("+", self, o)
    def __radd__(self, o): return self._op("+", o, self)
    def __sub__(self, o): return self._op("-", self, o)
    def __rsub__(self, o): return self._op("-", o, self)
    def __mul__(self, o): return self._op("*", self, o)
    def __rmul__(self, o): return self._op("*", o, self)
    def __truediv__(self, o): return self._op("/", self, o)
    def __rtruediv__(self, o): return self._op("/", o, self)
    def __neg__(self): return self._op("neg", self)
    def __pos__(self): return self
    def __abs__(self): return self._op("abs", self)
    def __lt__(self, o): return self._op("<", self, o)
    def __le__(self, o): return self._op("<=", self, o)
    def __gt__(self, o): return self._op(">", self, o)
    def __ge__(self, o): return self._op(">=", self, o)

    def __pow__(self, e):
        # Base.literal_pow (intfuncs.jl): x^0 = one(x), x^1 = x, x^2 = x*x, x^3 = x*x*x, x^-1 = inv(x), x^-2 = (i = inv(x); i*i) for a literal
        # integer exponent; anything else is pow
        if isinstance(e, int) and not isinstance(e, bool) and -2 <= e <= 3:
            if e == 0:
                return Symbol(self.trace, self.trace.emit("const", imm=1.0))
            if e == 1:
                return self
            if e == 2:
                return self * self
            if e == 3:
                return (self * self) * self
            inv = 1.0 / self
            return inv if e == -1 else inv * inv
        return self._op("pow", self, e)

    def __rpow__(self, base): return self._op("pow", base, self)

    def __bool__(self):
        raise TypeError("the truth value of a symbol of a boundary function is not known while the function is recorded: write "
                        "ocn.ifelse(condition, a, b) instead of `if condition:` (and ocn.min_ / ocn.max_ instead of the builtins min / max)")

    def __repr__(self):
        return f"Symbol(%{self.index})" if self.index is not None else f"Symbol({OP_NAMES[OPS[self.leaf[0]]]} {self.leaf[1]})"


def _symbolic(*xs):
    for x in xs:
        if isinstance(x, Symbol):
            return x
    return None


def _unary(name, on_numbers):
    def f(x):
        s = _symbolic(x)
        if s is None and hasattr(x, "grid"):          # a Field or an operation: the UnaryOperation of diagnostics.py
            from .diagnostics import unary_operation
            return unary_operation(name, x)
        return s._op(name, x) if s is not None else on_numbers(x)
    f.__name__ = name
    f.__doc__ = (f"{name}(x): one recorded instruction on a symbol of a traced function, a UnaryOperation on a Field or an operation, numpy's "
                 f"{name} on numbers and arrays")
    return f


sqrt = _unary("sqrt", np.sqrt)
exp = _unary("exp", np.exp)
log = _unary("log", np.log)
sin = _unary("sin", np.sin)
cos = _unary("cos", np.cos)
tanh = _unary("tanh", np.tanh)


def min_(a, b):
    """min(a, b) as Julia's (NaN propagates): one recorded instruction on symbols, numpy.minimum on numbers and arrays"""
    s = _symbolic(a, b)
    return s._op("min", a, b) if s is not None else np.minimum(a, b)


def max_(a, b):
    """max(a, b) as Julia's (NaN propagates): one recorded instruction on symbols, numpy.maximum on numbers and arrays"""
    s = _symbolic(a, b)
    return s._op("max", a, b) if s is not None else np.maximum(a, b)


def ifelse(condition, a, b):
    """ifelse(condition, a, b): both branches are evaluated, one is selected -- one recorded instruction on symbols, numpy.where on
    numbers and arrays"""
    s = _symbolic(condition, a, b)
    if s is not None:
        return s._op("select", condition, a, b)
    if np.ndim(condition) == 0 and np.ndim(a) == 0 and np.ndim(b) == 0:
        return a if condition else b
    return np.where(condition, a, b)


class ContinuousBoundaryFunction:
    """ContinuousBoundaryFunction(func, parameters, field_dependencies) (continuous_boundary_function.jl:22-44): the location-less
    descriptor a FluxBoundaryCondition(func, ...) holds until the model regularises it"""

    def __init__(self, func, parameters=None, field_dependencies=None):
        if not callable(func):
            raise TypeError("func must be callable")
        deps = (field_dependencies,) if isinstance(field_dependencies, str) else tuple(field_dependencies or ())       # tupleit
        self.func, self.parameters = func, parameters
        self.field_dependencies = tuple(str(d).lstrip(":") for d in deps)
        if len(self.field_dependencies) > MAX_DEPENDENCIES:
            raise ValueError(f"{len(self.field_dependencies)} field dependencies: the limit of a boundary function is {MAX_DEPENDENCIES} dependencies")

    def __repr__(self):
        return f"ContinuousBoundaryFunction {getattr(self.func, '__name__', 'func')} with field_dependencies {self.field_dependencies}"


def assumed_field_location(name):
    """assumed_field_location (Fields/field_tuples.jl): u, v, w on their faces, everything else at cell centres"""
    return {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}.get(name, (Center, Center, Center))


def tangential_directions(side):
    """the two tangential directions of side 0..5, x before y before z"""
    d = side // 2
    return (1, 2) if d == 0 else ((0, 2) if d == 1 else (0, 1))


class RegularizedBoundaryFunction:
    """regularize_boundary_condition(::ContinuousBoundaryFunction, grid, loc, dim, Side, field_names) (continuous_boundary_function.jl:
    76-92): the location with Nothing along the wall normal, the dependencies' interpolation operators to it, and the recorded program"""

    def __init__(self, cbf, grid, loc, side, field_names):
        from .diagnostics import interpolation_operator
        self.func, self.parameters, self.field_dependencies = cbf.func, cbf.parameters, cbf.field_dependencies
        self.side = int(side)
        d = self.side // 2
        self.location = tuple(None if q == d else l for q, l in enumerate(loc))
        missing = [n for n in self.field_dependencies if n not in field_names]
        if missing:
            # index_and_interp_dependencies (Utils/user_function_arguments.jl) fails on the first dependency that is no model field
            raise ValueError(f"field_dependencies {tuple(self.field_dependencies)} must be a subset of the model fields {tuple(field_names)}; "
                             f"{missing[0]} is not a model field")
        self.dependency_locations = tuple(assumed_field_location(n) for n in self.field_dependencies)
        topo = getattr(grid, "local", grid).topology
        # no interpolation along the normal (its location is Nothing) nor along a Flat direction (interpolation_operators.jl:87-110)
        self.interps = tuple(interpolation_operator(tuple(f if (q != d and topo[q] is not Flat) else None for q, f in enumerate(frm)),
                                                    tuple(l if (q != d and topo[q] is not Flat) else None for q, l in enumerate(loc)))
                             for frm in self.dependency_locations)
        self.coordinates = tuple(q for q in tangential_directions(self.side) if topo[q] is not Flat)      # X: the Flat ones dropped
        self.program = trace(self.func, [tangential_directions(self.side).index(q) for q in self.coordinates], len(self.field_dependencies),
                             self.parameters)
        self.reads_time = any(ins[0] == OPS["time"] for ins in self.program)


def trace(func, coordinates, ndeps, parameters=None):
    """call func(X..., t, deps..., [parameters]) once with symbols; `coordinates`: for every X the direction it is the node of -- the
    tangential direction 0 / 1 of a boundary function, x / y / z = 0 / 1 / 2 of a function in the volume (forcings.py). Returns the
    program, a list of (op, a, b, c, imm)."""
    if ndeps > MAX_DEPENDENCIES:
        raise ValueError(f"{ndeps} field dependencies: the limit of a traced function is {MAX_DEPENDENCIES} dependencies")
    tr = _Trace()
    args = [Symbol(tr, leaf=("coord", c)) for c in coordinates] + [Symbol(tr, leaf=("time",))] + [Symbol(tr, leaf=("field", s)) for s in range(ndeps)]
    if parameters is not None:
        args.append(parameters)
    result = func(*args)
    if isinstance(result, Symbol):
        last = tr.value(result)
        if last != len(tr.instructions) - 1:
            tr.emit("max", last, last)          # the flux is the LAST value: max(x, x) is x, bit for bit
    else:
        tr.value(result)                        # a plain number: a one-instruction program (anything else: TypeError)
        tr.instructions = tr.instructions[-1:]
    return tr.instructions


def interpret(program, coordinates, time, deps):
    """a program on numpy arrays, operation by operation (host twin of the device interpreters): coordinates[a] and deps[slot] are
    arrays that broadcast against each other"""
    with np.errstate(all="ignore"):
        v = []
        for op, a, b, c, imm in program:
            k = OP_NAMES[op]
            if k == "const":
                r = np.float64(imm)
            elif k == "coord":
                r = coordinates[a]
            elif k == "time":
                r = np.float64(time)
            elif k == "field":
                r = deps[a]
            elif k in ("<", "<=", ">", ">="):
                r = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}[k](v[a], v[b]).astype(np.float64)
            elif k == "select":
                r = np.where(v[a] != 0.0, v[b], v[c])
            elif k in ("+", "-", "*", "/", "min", "max", "pow"):
                r = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "min": np.minimum, "max": np.maximum,
                     "pow": np.power}[k](v[a], v[b])
            else:
                r = {"neg": np.negative, "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos,
                     "tanh": np.tanh}[k](v[a])
            v.append(r)
        return v[-1]


def program_array(program):
    """the ctypes array of ocn_expr_ins_t of a program, and its length"""
    from . import _lib
    arr = (_lib.ExprIns * max(len(program), 1))()
    for q, (op, a, b, c, imm) in enumerate(program):
        arr[q].op, arr[q].a, arr[q].b, arr[q].c, arr[q].imm = int(op), int(a), int(b), int(c), float(imm)
    return arr, len(program)
