"""Fields (reference: src/Fields/field.jl:23-38, src/Grids/new_data.jl:36-73).

A Field owns (or borrows) a dense device array WITH halos in the reference's parent layout: column-major, x fastest,
interior element (i, j, k) at (i-1+Hx, j-1+Hy, k-1+Hz)."""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Bounded, Center, Face

_LOC_CODE = {Center: 0, Face: 1}


class Field:
    """Field(loc, grid, data=None) -- or Field(operand, compute=True) for a BinaryOperation or a scan (Average, Integral, Reduction,
    CumulativeIntegral, Accumulation): the computed field of AbstractOperations/computed_field.jl:42-72 and Fields/scans.jl:45-72,
    whose `operand` ocn.compute(field) evaluates (diagnostics.py)"""

    __array_ufunc__ = None    # a numpy scalar on the left of an operation defers to the reflected method

    def __init__(self, loc, grid=None, data=None, owner=None, compute=True):
        operand = None
        if not isinstance(loc, (tuple, list)):
            from . import diagnostics
            operand = diagnostics.as_field_operand(loc)
            if grid is not None or data is not None:
                raise NotImplementedError("Field(operand): the computed field allocates its own data on the operand's grid")
            loc, grid = operand.location, operand.grid
        self.grid = grid
        self.loc = tuple(loc)
        self.shape = grid.total_size(self.loc)
        self.nbytes = int(np.prod(self.shape)) * 8
        self._owner = None   # views into a model's memory do NOT keep the model alive (no reference cycles)
        self.operand = operand
        self.status = None
        if data is None:
            p = C.c_void_p()
            _lib.check(_lib.lib().ocn_malloc(C.byref(p), self.nbytes))   # zeros(arch, FT, sz...)
            self.data = p
            self._owns = True
        else:
            self.data = data if isinstance(data, C.c_void_p) else C.c_void_p(data)
            self._owns = False
        if operand is not None:
            from . import diagnostics
            self.status = diagnostics.FieldStatus()
            if compute:
                diagnostics.compute(self)

    @property
    def architecture(self):
        return self.grid.architecture

    @property
    def loc_codes(self):
        return tuple(_LOC_CODE[l] for l in self.loc)

    # ---- host transfers ------------------------------------------------------------------------------------------
    def parent(self):
        """Array(parent(field)): host copy of the whole haloed array (Fortran order)."""
        a = np.empty(self.shape, dtype=np.float64, order="F")
        _lib.check(_lib.lib().ocn_memcpy_d2h(a.ctypes.data, self.data, self.nbytes))
        return a

    def set_parent(self, a):
        a = np.asfortranarray(a, dtype=np.float64)
        if a.shape != self.shape:
            raise ValueError(f"parent shape {a.shape} != {self.shape}")
        _lib.check(_lib.lib().ocn_memcpy_h2d(self.data, a.ctypes.data, self.nbytes))

    def _interior_slices(self):
        g = self.grid
        return tuple(slice(0, 1) if l is None else slice(h, h + n) for h, n, l in zip(g.halo_size, g.interior_size(self.loc), self.loc))

    def interior(self):
        """Array(interior(field)) (field.jl: interior)"""
        return self.parent()[self._interior_slices()]

    def set(self, value):
        """set!(field, value): value is an array of interior size, a number, or f(x, y, z)."""
        a = self.parent()
        view = a[self._interior_slices()]
        if callable(value):
            x, y, z = self.grid.nodes(self.loc)
            view[...] = value(x, y, z)
        else:
            view[...] = value
        self.set_parent(a)
        return self

    # ---- operations and reductions (diagnostics.py): descriptors, no device work until Field(op) / compute; see _add_operations below ----

    def __del__(self):
        if getattr(self, "_owns", False):
            try:
                _lib.lib().ocn_free(self.data)
            except Exception:
                pass


def _add_operations():
    """the operators (a BinaryOperation descriptor each) and the allocating reductions of Field, forwarded to diagnostics.py"""
    def binary(symbol, reflected):
        def method(self, other):
            from .diagnostics import binary_operation
            return binary_operation(symbol, other, self) if reflected else binary_operation(symbol, self, other)
        return method

    def reduction(name):
        def method(self, dims=None, **kw):
            from . import diagnostics
            return getattr(diagnostics, name)(self, dims=dims, **kw)
        method.__name__ = name
        return method

    def power(self, exponent):
        from .diagnostics import power
        return power(self, exponent)

    for name, symbol in (("add", "+"), ("sub", "-"), ("mul", "*"), ("truediv", "/")):
        setattr(Field, f"__{name}__", binary(symbol, False))
        setattr(Field, f"__r{name}__", binary(symbol, True))
    Field.__pow__ = power

    def unary(name):
        def method(self):
            from .diagnostics import unary_operation
            return unary_operation(name, self)
        return method
    Field.__neg__, Field.__abs__ = unary("neg"), unary("abs")
    for name in ("sum", "mean", "maximum", "minimum"):       # maximum / minimum also take f = None | abs
        setattr(Field, name, reduction(name))


_add_operations()


def CenterField(grid):
    return Field((Center, Center, Center), grid)


def XFaceField(grid):
    return Field((Face, Center, Center), grid)


def YFaceField(grid):
    return Field((Center, Face, Center), grid)


def ZFaceField(grid):
    return Field((Center, Center, Face), grid)


def interior(field):
    return field.interior()


def set_(field, value):
    return field.set(value)


def _ptr_array(fields):
    return (C.c_void_p * len(fields))(*[f.data for f in fields])


def _loc_array(fields):
    arr = ((C.c_int * 3) * len(fields))()
    for n, f in enumerate(fields):
        for d in range(3):
            arr[n][d] = f.loc_codes[d]
    return arr


def fill_halo_regions(fields, fill_open_bcs=True, boundary_conditions=None):
    """fill_halo_regions!(field | tuple of fields; fill_open_bcs) (BoundaryConditions/fill_halo_regions.jl:25-36) with the
    default boundary conditions (field_boundary_conditions.jl:15-25) or, per field, a FieldBoundaryConditions of constant
    Flux / Value / Gradient / Open conditions (`boundary_conditions`: one entry or None per field)."""
    if isinstance(fields, Field):
        fields = [fields]
        if boundary_conditions is not None and not isinstance(boundary_conditions, (list, tuple)):
            boundary_conditions = [boundary_conditions]
    fields = list(fields)
    if not fields:
        return
    grid = fields[0].grid
    if boundary_conditions is None:
        _lib.check(_lib.lib().ocn_fill_halo_regions(grid.handle, _ptr_array(fields), _loc_array(fields), len(fields),
                                                    int(fill_open_bcs)))
        return
    from .boundary_conditions import bc_table
    if len(boundary_conditions) != len(fields):
        raise ValueError("one FieldBoundaryConditions (or None) per field")
    _lib.check(_lib.lib().ocn_fill_halo_regions_bcs(grid.handle, _ptr_array(fields), _loc_array(fields), len(fields),
                                                    bc_table(list(boundary_conditions), grid), int(fill_open_bcs)))
