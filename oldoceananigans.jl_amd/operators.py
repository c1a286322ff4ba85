"""Operators on a RectilinearGrid and the recorder of stencil programs (reference: src/Operators/, src/AbstractOperations/
kernel_function_operation.jl:58-70).

    from oldoceananigans_jl_amd.operators import ζ3ᶠᶠᶜ
    ζ = ocn.Field(ocn.KernelFunctionOperation((ocn.Face, ocn.Face, ocn.Center), ζ3ᶠᶠᶜ, grid, u, v))

A kernel function f(i, j, k, grid, args...) cannot cross the C ABI; a program can (boundary_functions.py). The function is called ONCE
with symbols: i, j, k are index symbols (`i + 1`, `k - 1` and nothing else), every Field argument a field symbol whose
u[i + 1, j, k] records a load at a constant offset and returns a value with all the arithmetic of a boundary function's symbols. The
record is a straight-line program of ocn_stencil_ins_t (include/ocn_mi355x.h) with VALUE NUMBERING: the same (op, operands) and the same
load (slot, di, dj, dk) are emitted once -- the same operation on the same bits gives the same bits, so nothing changes numerically, and
operators that call operators at shifted indices do not explode. Nothing is simplified or reassociated.

The operators below are the reference's, written as the reference writes them and generated over the location superscripts in loops as
the reference does with @eval. Each takes a field symbol or a function f(i, j, k, grid, args...) (the reference's two methods). Names are
the reference's wherever Python accepts them as identifiers; `∂`, `⁻¹` and `₃` are not: ∂xᶜᶜᶜ is dxᶜᶜᶜ, Δx⁻¹ᶜᶜᶜ is Δx_invᶜᶜᶜ, ζ₃ᶠᶠᶜ is
ζ3ᶠᶠᶜ (every docstring carries the reference's name). x and y are regular here, so Δx and Δy are numbers; Δz of a stretched grid is the
grid's table at k + dk. Flat directions follow the reference's Flat methods: δ is zero, ℑ the identity, Δ is 1."""
import numbers
import struct
import unicodedata

import numpy as np

from . import boundary_functions as _bf
from .boundary_functions import Symbol
from .grids import Center, Face, Flat

MAX_INSTRUCTIONS = 256        # OCN_STENCIL_MAX_INSTRUCTIONS
MAX_SLOTS = 64                # OCN_STENCIL_MAX_SLOTS: values alive at once
MAX_ARGUMENTS = 8             # OCN_STENCIL_MAX_ARGUMENTS

# the arithmetic of OCN_EXPR_* and the leaves of a stencil program (include/ocn_mi355x.h); no coord, time, field
OPS = {k: v for k, v in _bf.OPS.items() if k not in ("coord", "time", "field")}
OPS.update({"load": 25, "spacing": 26, "node": 27})
OP_NAMES = {v: k for k, v in OPS.items()}
ARITY = {"const": 0, "load": 0, "spacing": 0, "node": 0, "neg": 1, "abs": 1, "sqrt": 1, "exp": 1, "log": 1, "sin": 1, "cos": 1, "tanh": 1,
         "+": 2, "-": 2, "*": 2, "/": 2, "min": 2, "max": 2, "pow": 2, "<": 2, "<=": 2, ">": 2, ">=": 2, "select": 3}

_INDEX_MESSAGE = ("an index symbol (i, j, k of a kernel function) used as a number: it supports `± int` only and may be passed to "
                  "operators and to the [] of a field argument")
_FIELD_MESSAGE = "a field symbol used without indexing: write u[i, j, k] (or pass it to an operator)"


# ---------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------
class StencilTrace(_bf._Trace):
    """the instructions recorded so far: tuples (op, a, b, c, di, dj, dk, imm), each distinct one once"""

    def __init__(self):
        self.instructions = []
        self.numbered = {}

    def emit(self, op, a=0, b=0, c=0, imm=0.0, offset=(0, 0, 0)):
        ins = (OPS[op], int(a), int(b), int(c), int(offset[0]), int(offset[1]), int(offset[2]), float(imm))
        key = ins[:7] + (struct.pack("<d", ins[7]),)          # the bits of the constant: -0.0 is not 0.0
        if key in self.numbered:
            return self.numbered[key]
        return self.append(ins, key)

    def append(self, ins, key=None):
        if len(self.instructions) == MAX_INSTRUCTIONS:
            raise ValueError(f"the function performs more than {MAX_INSTRUCTIONS} distinct operations: the limit of a stencil program is "
                             f"{MAX_INSTRUCTIONS} instructions")
        self.instructions.append(ins)
        if key is not None:
            self.numbered[key] = len(self.instructions) - 1
        return len(self.instructions) - 1

    def value(self, x):
        if isinstance(x, Index):
            raise TypeError(_INDEX_MESSAGE)
        if isinstance(x, FieldSymbol):
            raise TypeError(_FIELD_MESSAGE)
        return super().value(x)


def _refusing(message):
    def method(self, *_):
        raise TypeError(message)
    return method


class Index:
    """i, j or k of a kernel function: a direction and a constant offset"""

    __array_ufunc__ = None

    def __init__(self, axis, offset=0):
        self.axis, self.offset = axis, offset

    def _shifted(self, n, sign):
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (numbers.Integral, np.integer)):
            raise TypeError(_INDEX_MESSAGE)
        return Index(self.axis, self.offset + sign * int(n))

    def __add__(self, n): return self._shifted(n, 1)
    __radd__ = __add__
    def __sub__(self, n): return self._shifted(n, -1)

    def __repr__(self):
        return "ijk"[self.axis] + (f"{self.offset:+d}" if self.offset else "")


class FieldSymbol:
    """a Field argument of a kernel function: argument slot `slot` at `loc`; u[i + di, j + dj, k + dk] records a load"""

    __array_ufunc__ = None

    def __init__(self, trace, slot, loc):
        self.trace, self.slot, self.loc = trace, slot, tuple(loc)

    def __getitem__(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 3 and all(isinstance(x, Index) and x.axis == d for d, x in enumerate(idx))):
            raise TypeError("a field symbol is indexed with the three index symbols and constant offsets: u[i + 1, j, k]")
        return Symbol(self.trace, self.trace.emit("load", a=self.slot, offset=tuple(x.offset for x in idx)))

    def __repr__(self):
        return f"FieldSymbol(slot {self.slot})"


for _name in ("rsub", "mul", "rmul", "truediv", "rtruediv", "floordiv", "mod", "neg", "pos", "abs", "pow", "rpow", "lt", "le", "gt", "ge", "float",
              "int", "index", "bool"):
    setattr(Index, f"__{_name}__", _refusing(_INDEX_MESSAGE))
for _name in ("add", "radd", "sub", "rsub", "mul", "rmul", "truediv", "rtruediv", "neg", "pos", "abs", "pow", "rpow", "lt", "le", "gt", "ge", "float",
              "int", "bool"):
    setattr(FieldSymbol, f"__{_name}__", _refusing(_FIELD_MESSAGE))


class StencilProgram:
    """a recorded program with what it reads: `fields` (argument slot -> Field) and the `location` it is evaluated at"""

    def __init__(self, program, fields, location, grid):
        self.program, self.fields, self.location, self.grid = list(program), list(fields), tuple(location), grid
        check_reach(self.program, grid, self.location, [f.loc for f in self.fields])
        self.slots, self.nslots = plan(self.program, len(self.fields))


def record(function, grid, location, arguments=()):
    """call function(i, j, k, grid, *arguments) once with symbols -- every Field among `arguments` replaced by a field symbol, everything
    else handed over untouched -- and return the StencilProgram. ValueError: a limit or the reach rule; TypeError: a misused symbol."""
    from .fields import Field
    tr = StencilTrace()
    fields, call = [], []
    for a in arguments:
        if isinstance(a, Field):
            if not any(a is f for f in fields):
                fields.append(a)
            slot = next(q for q, f in enumerate(fields) if a is f)
            call.append(FieldSymbol(tr, slot, a.loc))
        else:
            call.append(a)
    if len(fields) > MAX_ARGUMENTS:
        raise ValueError(f"{len(fields)} field arguments: the limit of a stencil program is {MAX_ARGUMENTS} arguments")
    _TRACES.append(tr)
    try:
        result = function(Index(0), Index(1), Index(2), grid, *call)
    finally:
        _TRACES.pop()
    if isinstance(result, Symbol):
        last = tr.value(result)
        if last != len(tr.instructions) - 1:                  # the operand is the LAST value: max(x, x) is x, bit for bit
            tr.append((OPS["max"], last, last, 0, 0, 0, 0, 0.0))
    else:
        tr.value(result)                                      # a plain number: a one-instruction program (anything else: TypeError)
        tr.instructions = tr.instructions[-1:]
    return StencilProgram(tr.instructions, fields, location, grid)


def _interior(grid, loc):
    return grid.interior_size(loc)


def check_reach(program, grid, location, arg_locs):
    """the reach rule of include/ocn_mi355x.h, restated: a recorded offset never becomes an out-of-bounds read. For a LOAD along a
    non-Flat direction d, with n_out the interior extent of `location` and n_arg that of the argument: off >= -H_d and
    n_out + off <= n_arg + H_d. ValueError names the argument, the direction and the halo it would need."""
    nout, H, N = _interior(grid, location), grid.halo_size, grid.size
    for q, (op, a, b, _c, di, dj, dk, _imm) in enumerate(program):
        kind, off = OP_NAMES.get(op), (di, dj, dk)
        if kind == "load":
            narg = _interior(grid, arg_locs[a])
            for d in range(3):
                if grid.topology[d] is Flat:
                    if off[d]:
                        raise ValueError(f"instruction {q}: argument {a} is read at offset {off[d]:+d} along {'xyz'[d]}, which is Flat")
                    continue
                need = max(-off[d], nout[d] + off[d] - narg[d])
                if need > H[d]:
                    raise ValueError(f"instruction {q}: argument {a} read at offset {off[d]:+d} along {'xyz'[d]} ({nout[d]} output points, {narg[d]} "
                                     f"of the argument) needs a halo of {need}; the grid has {H[d]}")
        elif kind == "spacing" and a == 2 and grid.topology[2] is not Flat:
            need = max(-dk, nout[2] + dk - (N[2] + 1))
            if need > H[2]:
                raise ValueError(f"instruction {q}: Δz read at offset {dk:+d} along z ({nout[2]} output points) needs a halo of {need}; the grid has {H[2]}")
        elif kind == "node":
            n = 1 if grid.topology[a] is Flat else N[a] + (1 if b == 1 else 0)
            if off[a] < 0 or nout[a] + off[a] > n:
                raise ValueError(f"instruction {q}: the {'xyz'[a]} node at offset {off[a]:+d} ({nout[a]} output points) lies outside the {n} interior "
                                 "nodes of the table")


def program_array(program):
    """the ctypes array of ocn_stencil_ins_t of a program, and its length"""
    from . import _lib
    arr = (_lib.StencilIns * max(len(program), 1))()
    for q, (op, a, b, c, di, dj, dk, imm) in enumerate(program):
        I = arr[q]
        I.op, I.a, I.b, I.c, I.di, I.dj, I.dk, I.imm = int(op), int(a), int(b), int(c), int(di), int(dj), int(dk), float(imm)
    return arr, len(program)


def plan(program, nargs):
    """ocn_stencil_plan: the LDS slot of every value (a linear scan by last use) and the number of slots; host arithmetic of the library,
    no device. ValueError for what the library refuses (a malformed program, more than MAX_SLOTS values alive at once)."""
    import ctypes as C
    from . import _lib
    arr, n = program_array(program)
    slots, nslots = (C.c_int * max(n, 1))(), C.c_int(0)
    if _lib.lib().ocn_stencil_plan(arr, n, int(nargs), slots, C.byref(nslots)) != 0:
        raise ValueError(_lib.lib().ocn_last_error().decode())
    return list(slots)[:n], nslots.value


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------
_CODES = ("ᶜ", "ᶠ")
_ANY = "ᵃ"
__all__ = []


def _define(name, function, reference_name, where):
    """one function object per spelling, so that each carries its own name and the reference's"""
    def operator(*args):
        return function(*args)
    operator.__name__ = operator.__qualname__ = name
    operator.__doc__ = f"{reference_name} ({where})"
    # Python folds identifiers to NFKC: `dxᶜᶜᶜ` in source IS the name `dxccc`, `ℑxᶜᵃᵃ` is `Ixcaa`. Both spellings are bound, so that
    # attribute syntax and getattr(operators, "ℑxᶜᵃᵃ") find the same function
    globals()[name] = globals()[unicodedata.normalize("NFKC", name)] = operator
    __all__.append(unicodedata.normalize("NFKC", name))
    return operator


def _names(prefix, d, own):
    """every spelling of an operator along direction d that sits at `own` there: ᶜ / ᶠ / ᵃ in the two other places"""
    out = []
    for p in (_ANY,) + _CODES:
        for q in (_ANY,) + _CODES:
            sup = [p, q]
            sup.insert(d, own)
            out.append(prefix + "".join(sup))
    return out


def _value(f, i, j, k, grid, args):
    """f at (i, j, k): getindex of a field symbol, a call of a function, or the number itself"""
    if isinstance(f, FieldSymbol):
        return f[i, j, k]
    if callable(f):
        return f(i, j, k, grid, *args)
    return f


def _shift(ijk, d, n):
    return tuple(x + n if q == d and n else x for q, x in enumerate(ijk))


def _is_number(x):
    return isinstance(x, (numbers.Real, np.floating, np.integer)) and not isinstance(x, (Symbol, Index))


def _difference(d, own):
    lo, hi = (0, 1) if own == "ᶜ" else (-1, 0)

    def δ(i, j, k, grid, f, *args):
        if grid.topology[d] is Flat:
            return 0.0
        return _value(f, *_shift((i, j, k), d, hi), grid, args) - _value(f, *_shift((i, j, k), d, lo), grid, args)
    return δ


def _interpolation(d, own):
    lo, hi = (0, 1) if own == "ᶜ" else (-1, 0)

    def ℑ(i, j, k, grid, f, *args):
        if _is_number(f):
            return f
        if grid.topology[d] is Flat:
            return _value(f, i, j, k, grid, args)
        return 0.5 * (_value(f, *_shift((i, j, k), d, lo), grid, args) + _value(f, *_shift((i, j, k), d, hi), grid, args))
    return ℑ


def _spacing(d, own):
    def Δ(i, j, k, grid):
        if grid.topology[d] is Flat:
            return 1.0
        if d == 0:
            return float(grid.Δxᶜᵃᵃ)
        if d == 1:
            return float(grid.Δyᵃᶜᵃ)
        if grid.z_regular:
            return float(grid.Δzᵃᵃᶜ[0])
        if not isinstance(k, Index):
            raise TypeError("a spacing is asked for at the index symbols of the kernel function")
        # NOT value-numbered through the Python float: the grid's table at k + dk
        trace = _current_trace()
        return Symbol(trace, trace.emit("spacing", a=2, b=0 if own == "ᶜ" else 1, offset=(0, 0, k.offset)))
    return Δ


_TRACES = []


def _current_trace():
    if not _TRACES:
        raise TypeError("Δz of a stretched grid and the node operators record an instruction: call them inside a kernel function that is "
                        "being recorded (KernelFunctionOperation)")
    return _TRACES[-1]


_DIRS = "xyz"
_base = {}        # (family, d, own) -> function
for _d in range(3):
    for _own in _CODES:
        # δxᶜᵃᵃ .. δzᵃᵃᶠ and their 3D spellings (difference_operators.jl:7-27, Flat :33-49, 3D :55-73)
        _f = _difference(_d, _own)
        _base["δ", _d, _own] = _f
        for _n in _names("δ" + _DIRS[_d], _d, _own):
            _define(_n, _f, _n, "Operators/difference_operators.jl:7-73")
        # ℑxᶜᵃᵃ .. ℑzᵃᵃᶠ (interpolation_operators.jl:8-39, Flat :87-112)
        _f = _interpolation(_d, _own)
        _base["ℑ", _d, _own] = _f
        _sup = [_ANY, _ANY]
        _sup.insert(_d, _own)
        _define("ℑ" + _DIRS[_d] + "".join(_sup), _f, "ℑ" + _DIRS[_d] + "".join(_sup), "Operators/interpolation_operators.jl:8-39,87-112")
        # Δxᶜᵃᵃ .. Δzᶠᶠᶠ (spacings_and_areas_and_volumes.jl:44-145) and Δx⁻¹... = 1 / Δx... (reciprocal_metric_operators.jl:2-9)
        _f = _spacing(_d, _own)
        _base["Δ", _d, _own] = _f
        _r = (lambda Δ: lambda i, j, k, grid: 1 / Δ(i, j, k, grid))(_f)
        _base["Δ_inv", _d, _own] = _r
        for _n in _names("Δ" + _DIRS[_d], _d, _own):
            _define(_n, _f, _n, "Operators/spacings_and_areas_and_volumes.jl:44-145")
            _define(_n.replace("Δ" + _DIRS[_d], "Δ" + _DIRS[_d] + "_inv"), _r, _n.replace("Δ" + _DIRS[_d], "Δ" + _DIRS[_d] + "⁻¹"),
                    "Operators/reciprocal_metric_operators.jl:2-9")
        # ∂xᶜᵃᵃ .. ∂zᶠᶠᶠ: difference * reciprocal spacing, in that order (derivative_operators.jl:5-39)
        _dif, _rcp = _base["δ", _d, _own], _r

        def _derivative(i, j, k, grid, c, *args, _dif=_dif, _rcp=_rcp):
            if _is_number(c):
                return 0.0
            return _dif(i, j, k, grid, c, *args) * _rcp(i, j, k, grid)
        _base["∂", _d, _own] = _derivative
        for _n in _names("d" + _DIRS[_d], _d, _own):
            _define(_n, (lambda f: lambda i, j, k, grid, c, *args: f(i, j, k, grid, c, *args))(_derivative), "∂" + _n[1:],
                    "Operators/derivative_operators.jl:5-39")


def _compose(outer, inner):
    return lambda i, j, k, grid, f, *args: outer(i, j, k, grid, inner, f, *args)


# double interpolation: the higher direction outside (interpolation_operators.jl:45-56); triple: x of y of z (:62-71)
for _p in _CODES:
    for _q in _CODES:
        _define(f"ℑxy{_p}{_q}ᵃ", _compose(_base["ℑ", 1, _q], _base["ℑ", 0, _p]), f"ℑxy{_p}{_q}ᵃ", "Operators/interpolation_operators.jl:45-48")
        _define(f"ℑxz{_p}ᵃ{_q}", _compose(_base["ℑ", 2, _q], _base["ℑ", 0, _p]), f"ℑxz{_p}ᵃ{_q}", "Operators/interpolation_operators.jl:49-52")
        _define(f"ℑyzᵃ{_p}{_q}", _compose(_base["ℑ", 2, _q], _base["ℑ", 1, _p]), f"ℑyzᵃ{_p}{_q}", "Operators/interpolation_operators.jl:53-56")
        for _r3 in _CODES:
            _define(f"ℑxyz{_p}{_q}{_r3}",
                    (lambda X, Y, Z: lambda i, j, k, grid, f, *args: X(i, j, k, grid, Y, Z, f, *args))(_base["ℑ", 0, _p], _base["ℑ", 1, _q], _base["ℑ", 2, _r3]),
                    f"ℑxyz{_p}{_q}{_r3}", "Operators/interpolation_operators.jl:62-71")

# areas and volumes (spacings_and_areas_and_volumes.jl:294-335, 369-378), their reciprocals (reciprocal_metric_operators.jl:2-14) and the
# products metric * q (products_between_fields_and_grid_metrics.jl:5-14)
_metrics = {}
for _p in _CODES:
    for _q in _CODES:
        for _r3 in _CODES:
            _loc = _p + _q + _r3
            _Δx, _Δy, _Δz = _base["Δ", 0, _p], _base["Δ", 1, _q], _base["Δ", 2, _r3]
            _metrics["Δx" + _loc], _metrics["Δy" + _loc], _metrics["Δz" + _loc] = _Δx, _Δy, _Δz
            _metrics["Ax" + _loc] = (lambda a, b: lambda i, j, k, grid: a(i, j, k, grid) * b(i, j, k, grid))(_Δy, _Δz)
            _metrics["Ay" + _loc] = (lambda a, b: lambda i, j, k, grid: a(i, j, k, grid) * b(i, j, k, grid))(_Δx, _Δz)
            _metrics["Az" + _loc] = (lambda a, b: lambda i, j, k, grid: a(i, j, k, grid) * b(i, j, k, grid))(_Δx, _Δy)
            _metrics["V" + _loc] = (lambda a, b: lambda i, j, k, grid: a(i, j, k, grid) * b(i, j, k, grid))(_metrics["Az" + _loc], _Δz)
            for _m in ("Ax", "Ay", "Az", "V"):
                _f = _metrics[_m + _loc]
                _define(_m + _loc, _f, _m + _loc, "Operators/spacings_and_areas_and_volumes.jl:294-335,369-378")
                _define(_m + "_inv" + _loc, (lambda f: lambda i, j, k, grid: 1 / f(i, j, k, grid))(_f), _m + "⁻¹" + _loc,
                        "Operators/reciprocal_metric_operators.jl:2-14")
            for _m in ("Δx", "Δy", "Δz", "Ax", "Ay", "Az"):
                _define(_m + "_q" + _loc,
                        (lambda f: lambda i, j, k, grid, q, *args: f(i, j, k, grid) * _value(q, i, j, k, grid, args))(_metrics[_m + _loc]),
                        _m + "_q" + _loc, "Operators/products_between_fields_and_grid_metrics.jl:5-14")
    for _q in _CODES:
        _define(f"Az{_p}{_q}ᵃ", _metrics[f"Az{_p}{_q}ᶜ"], f"Az{_p}{_q}ᵃ", "Operators/spacings_and_areas_and_volumes.jl:306-311")


def divᶜᶜᶜ(i, j, k, grid, u, v, w):
    """divᶜᶜᶜ (Operators/divergence_operators.jl:16-19)"""
    return V_invᶜᶜᶜ(i, j, k, grid) * (δxᶜᶜᶜ(i, j, k, grid, Ax_qᶠᶜᶜ, u) + δyᶜᶜᶜ(i, j, k, grid, Ay_qᶜᶠᶜ, v) + δzᶜᶜᶜ(i, j, k, grid, Az_qᶜᶜᶠ, w))    # noqa: F821


def flux_div_xyᶜᶜᶜ(i, j, k, grid, u, v):
    """flux_div_xyᶜᶜᶜ (Operators/divergence_operators.jl:35-36)"""
    return δxᶜᶜᶜ(i, j, k, grid, Ax_qᶠᶜᶜ, u) + δyᶜᶜᶜ(i, j, k, grid, Ay_qᶜᶠᶜ, v)    # noqa: F821


def div_xyᶜᶜᶜ(i, j, k, grid, u, v):
    """div_xyᶜᶜᶜ (Operators/divergence_operators.jl:38-39)"""
    return V_invᶜᶜᶜ(i, j, k, grid) * flux_div_xyᶜᶜᶜ(i, j, k, grid, u, v)    # noqa: F821


def Γᶠᶠᶜ(i, j, k, grid, u, v):
    """Γᶠᶠᶜ (Operators/vorticity_operators.jl:2)"""
    return δxᶠᶠᶜ(i, j, k, grid, Δy_qᶜᶠᶜ, v) - δyᶠᶠᶜ(i, j, k, grid, Δx_qᶠᶜᶜ, u)    # noqa: F821


def ζ3ᶠᶠᶜ(i, j, k, grid, u, v):
    """ζ₃ᶠᶠᶜ (Operators/vorticity_operators.jl:9)"""
    return Γᶠᶠᶜ(i, j, k, grid, u, v) * Az_invᶠᶠᶜ(i, j, k, grid)    # noqa: F821


def _node(d):
    def node(i, j, k, grid, ℓx, ℓy, ℓz):
        ℓ = (ℓx, ℓy, ℓz)[d]
        ℓ = ℓ if isinstance(ℓ, type) else type(ℓ)
        if ℓ not in (Center, Face):
            raise TypeError(f"{'xyz'[d]}node: the location along {'xyz'[d]} is Center or Face")
        index = (i, j, k)[d]
        if not isinstance(index, Index):
            raise TypeError("a node is asked for at the index symbols of the kernel function")
        trace = _current_trace()
        offset = [0, 0, 0]
        offset[d] = index.offset
        return Symbol(trace, trace.emit("node", a=d, b=0 if ℓ is Center else 1, offset=offset))
    return node


xnode = _define("xnode", _node(0), "xnode(i, j, k, grid, ℓx, ℓy, ℓz)", "Grids/rectilinear_grid.jl:483")
ynode = _define("ynode", _node(1), "ynode(i, j, k, grid, ℓx, ℓy, ℓz)", "Grids/rectilinear_grid.jl:484")
znode = _define("znode", _node(2), "znode(i, j, k, grid, ℓx, ℓy, ℓz)", "Grids/vertical_discretization.jl:198")
for _name in ("divᶜᶜᶜ", "flux_div_xyᶜᶜᶜ", "div_xyᶜᶜᶜ", "Γᶠᶠᶜ", "ζ3ᶠᶠᶜ"):
    globals()[_name] = globals()[unicodedata.normalize("NFKC", _name)]
    __all__.append(unicodedata.normalize("NFKC", _name))


def identity(i, j, k, grid, f, *args):
    """identity1 .. identity5 (Operators/interpolation_utils.jl): what interpolation_operator answers where nothing moves"""
    return _value(f, i, j, k, grid, args)


def interpolation(name):
    """the operator interpolation_operator(from, to) NAMES (diagnostics.interpolation_operator), e.g. "ℑxzᶜᵃᶠ" """
    return identity if name == "identity" else globals()[name]
