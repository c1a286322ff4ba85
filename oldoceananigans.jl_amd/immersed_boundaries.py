"""ImmersedBoundaryGrid with grid-fitted boundaries (reference: src/ImmersedBoundaries/immersed_boundary_grid.jl, grid_fitted_bottom.jl,
grid_fitted_boundary.jl, mask_immersed_field.jl). The boundary is materialised on the host -- the numerical bottom height or the mask,
halos filled -- and handed to the library as one cell mask (ocn_grid_set_immersed_boundary), from which a kernel builds the two flag
tables every immersed kernel reads (csrc/ocn_immersed.h). Metrics, hydrostatic pressure and the pressure solve are the underlying
grid's."""
import ctypes as C

import numpy as np

from . import _lib
from .grids import Bounded, Center, Flat, FullyConnected, LeftConnected, RectilinearGrid, RightConnected

NAME = "ImmersedBoundaryGrid"


def refuse(feature):
    """what an immersed grid does not serve: the message names the grid and the feature"""
    raise NotImplementedError(f"{feature} is not served on an {NAME}")


def is_immersed(grid):
    return isinstance(getattr(grid, "local", grid), ImmersedBoundaryGrid)


class CenterImmersedCondition:
    """the cells whose CENTRE lies at or below the bottom are immersed (grid_fitted_bottom.jl:19)"""

    def __eq__(self, other):
        return type(other) is type(self)

    def __hash__(self):
        return hash(type(self))

    def __repr__(self):
        return type(self).__name__


class InterfaceImmersedCondition(CenterImmersedCondition):
    """the cells whose upper INTERFACE lies at or below the bottom are immersed (grid_fitted_bottom.jl:20)"""


def _same(a, b):
    """`==` of two bottom heights or masks: numbers and arrays by value, functions by identity"""
    if callable(a) or callable(b):
        return a is b
    if isinstance(a, HostField) or isinstance(b, HostField):
        return isinstance(a, HostField) and isinstance(b, HostField) and np.array_equal(a.parent(), b.parent())
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


class HostField:
    """a materialised bottom height (Center, Center, Nothing) or mask (Center, Center, Center): the parent array, halos filled, on the host"""

    def __init__(self, data, halo, loc):
        self._data, self._halo, self.loc = data, tuple(halo), loc

    def parent(self):
        return self._data

    def interior(self):
        sl = tuple(slice(h, n - h) for h, n in zip(self._halo, self._data.shape))
        return self._data[sl]


class GridFittedBottom:
    """GridFittedBottom(bottom_height, immersed_condition=CenterImmersedCondition()) (grid_fitted_bottom.jl:22-53): bottom_height is a
    number, an (Nx, Ny) array or a function of the non-Flat horizontal coordinates, in absolute z"""

    def __init__(self, bottom_height, immersed_condition=None):
        immersed_condition = CenterImmersedCondition() if immersed_condition is None else immersed_condition
        if isinstance(immersed_condition, type):
            immersed_condition = immersed_condition()
        if not isinstance(immersed_condition, CenterImmersedCondition):
            raise TypeError("immersed_condition is CenterImmersedCondition() or InterfaceImmersedCondition()")
        self.bottom_height, self.immersed_condition = bottom_height, immersed_condition

    def __eq__(self, other):
        """grid_fitted_bottom.jl:170-172"""
        return (isinstance(other, GridFittedBottom) and _same(self.bottom_height, other.bottom_height) and
                self.immersed_condition == other.immersed_condition)

    __hash__ = None

    def summary(self):
        """grid_fitted_bottom.jl:55-71"""
        h = self.bottom_height
        if callable(h):
            return f"GridFittedBottom({getattr(h, '__name__', h)})"
        a = h.interior() if isinstance(h, HostField) else np.asarray(h, dtype=np.float64)
        return f"GridFittedBottom(mean(z)={a.mean():.6g}, min(z)={a.min():.6g}, max(z)={a.max():.6g})"

    __repr__ = summary


class GridFittedBoundary:
    """GridFittedBoundary(mask) (grid_fitted_boundary.jl:10-12): mask is an (Nx, Ny, Nz) boolean array or a function of the non-Flat
    coordinates, true where a cell is immersed"""

    def __init__(self, mask):
        self.mask = mask

    def __eq__(self, other):
        return isinstance(other, GridFittedBoundary) and _same(self.mask, other.mask)

    __hash__ = None

    def summary(self):
        m = self.mask
        if callable(m):
            return f"GridFittedBoundary({getattr(m, '__name__', m)})"
        a = m.interior() if isinstance(m, HostField) else np.asarray(m)
        return f"GridFittedBoundary({int(np.count_nonzero(a))} of {a.size} cells immersed)"

    __repr__ = summary


def PartialCellBottom(*args, **kwargs):
    """PartialCellBottom(bottom_height; minimum_fractional_cell_height) (partial_cell_bottom.jl): not built"""
    refuse("PartialCellBottom (partial cells change the vertical metrics)")


class ImmersedBoundaryCondition:
    """ImmersedBoundaryCondition(; west, east, ...) (immersed_boundary_condition.jl): not built"""

    def __init__(self, *args, **kwargs):
        refuse("ImmersedBoundaryCondition (a boundary condition on the immersed boundary)")


def _fill_halo(a, d, H, topology):
    """fill_halo_regions! of a Center field with its default conditions along d: a Periodic copy, the no-flux mirror next to a wall
    (fill_halo_regions_periodic.jl:5-33, fill_halo_regions_flux.jl:9-27)"""
    if H == 0:
        return
    N = a.shape[d] - 2 * H
    lo = [slice(None)] * a.ndim
    src = [slice(None)] * a.ndim
    for h in range(1, H + 1):
        for side in (0, 1):
            wall = topology in (Bounded, RightConnected) if side == 0 else topology in (Bounded, LeftConnected)
            if side == 0:          # node 1 - h  <-  node N + 1 - h (Periodic) | node h (wall)
                lo[d], src[d] = H - h, (H + h - 1) if wall else (H + N - h)
            else:                  # node N + h  <-  node h (Periodic) | node N + 1 - h (wall)
                lo[d], src[d] = H + N + h - 1, (H + N - h) if wall else (H + h - 1)
            a[tuple(lo)] = a[tuple(src)]


def _horizontal_nodes(grid):
    """the Center nodes of the non-Flat horizontal directions as broadcastable (Nx, 1) / (1, Ny) arrays"""
    x, y, _ = grid.nodes((Center, Center, Center))
    return [c[:, :, 0] for c, t in zip((x, y), grid.topology[:2]) if t is not Flat]


def _values(value, shape, coordinates, what):
    """set!(field, value): a number, an array of the interior size (a trailing singleton allowed) or a function of the coordinates"""
    if callable(value):
        return np.broadcast_to(np.asarray(value(*coordinates)), shape)
    a = np.asarray(value)
    if a.ndim == 0:
        return np.broadcast_to(a, shape)
    if a.shape != shape and a.shape == shape + (1,):
        a = a[..., 0]
    if a.shape != shape and a.shape == tuple(n for n in shape if n != 1):
        a = a.reshape(shape)
    if a.shape != shape:
        raise ValueError(f"{what} has shape {a.shape}; the grid needs {shape}")
    return a


def numerical_bottom_height(grid, ib):
    """_compute_numerical_bottom_height! (grid_fitted_bottom.jl:111-122): the z face on top of the highest immersed cell of each column, the
    bottom face of the grid where none is; (Nx, Ny)"""
    Nx, Ny, Nz, Hz = grid.Nx, grid.Ny, grid.Nz, grid.Hz
    zb = np.array(_values(ib.bottom_height, (Nx, Ny), _horizontal_nodes(grid), "bottom_height"), dtype=np.float64)
    zf, zc = np.asarray(grid.zᵃᵃᶠ), np.asarray(grid.zᵃᵃᶜ)
    flat_z = grid.topology[2] is Flat
    face = (lambda k: zf[0]) if flat_z else (lambda k: zf[k - 1 + Hz])
    centre = (lambda k: zc[0]) if flat_z else (lambda k: zc[k - 1 + Hz])
    out = np.full((Nx, Ny), face(1), dtype=np.float64)
    interface = isinstance(ib.immersed_condition, InterfaceImmersedCondition)
    for k in range(1, Nz + 1):
        zp = face(k + 1)
        bottom_cell = (zp <= zb) if interface else (centre(k) <= zb)
        out = np.where(bottom_cell, zp, out)
    return out


class ImmersedBoundaryGrid(RectilinearGrid):
    """ImmersedBoundaryGrid(grid, ib) (immersed_boundary_grid.jl:33-60): `grid` with the grid-fitted boundary `ib` materialised on it
    (materialize_immersed_boundary, grid_fitted_bottom.jl:99-130, grid_fitted_boundary.jl:22-32). The object is a grid of its own -- its
    library handle carries the boundary --; `underlying_grid` is a plain grid of the same size, halo, topology and nodes."""

    def __init__(self, grid, ib, active_cells_map=False):
        if active_cells_map:
            refuse("active_cells_map=True (an active-cells map)")
        if hasattr(grid, "local") or any(t in (FullyConnected, RightConnected, LeftConnected) for t in grid.topology):
            refuse("a partitioned grid")
        if isinstance(grid, ImmersedBoundaryGrid):
            raise ValueError("ImmersedBoundaryGrids require a non-immersed underlying grid")
        if not isinstance(ib, (GridFittedBottom, GridFittedBoundary)):
            raise TypeError("the immersed boundary is a GridFittedBottom or a GridFittedBoundary")
        super().__init__(grid.architecture, halo=grid.halo_size, **grid._constructor_arguments)
        self._user_boundary = ib
        self._underlying = None
        P = tuple(n + 2 * h for n, h in zip(self.size, self.halo_size))
        if isinstance(ib, GridFittedBottom):
            zb = np.empty(P[:2], dtype=np.float64)
            zb[self.Hx:self.Hx + self.Nx, self.Hy:self.Hy + self.Ny] = numerical_bottom_height(self, ib)
            for d in (0, 1):
                _fill_halo(zb, d, self.halo_size[d], self.topology[d])
            self.immersed_boundary = GridFittedBottom(HostField(zb[:, :, None], (self.Hx, self.Hy, 0), (Center, Center, None)), ib.immersed_condition)
            # _immersed_cell (grid_fitted_bottom.jl:124-130): z_centre <= z_bottom, at every level the nodes are defined on, halos included
            zc = np.asarray(self.zᵃᵃᶜ, dtype=np.float64)
            self._cell = np.asfortranarray(zc[None, None, :P[2]] <= zb[:, :, None])
        else:
            nodes = [c for c, t in zip(self.nodes((Center, Center, Center)), self.topology) if t is not Flat]
            mask = np.zeros(P, dtype=bool)
            mask[self.Hx:self.Hx + self.Nx, self.Hy:self.Hy + self.Ny, self.Hz:self.Hz + self.Nz] = _values(ib.mask, self.size, nodes, "mask") != 0
            for d in range(3):
                _fill_halo(mask, d, self.halo_size[d], self.topology[d])
            self.immersed_boundary = GridFittedBoundary(HostField(mask, self.halo_size, (Center, Center, Center)))
            self._cell = np.asfortranarray(mask)

    @property
    def underlying_grid(self):
        if self._underlying is None:
            self._underlying = RectilinearGrid(self.architecture, halo=self.halo_size, **self._constructor_arguments)
        return self._underlying

    def immersed_cell_mask(self):
        """immersed_cell(i, j, k, ibg) over the parent extent at (Center, Center, Center), halos filled: a boolean array"""
        return self._cell.copy(order="F")

    def _with_halo(self, halo):
        """with_halo(halo, ibg) (immersed_boundary_grid.jl:93-98): the underlying grid with the new halo, the boundary materialised again"""
        from .grids import with_halo
        return ImmersedBoundaryGrid(with_halo(halo, self.underlying_grid), self._user_boundary)

    @property
    def handle(self):
        fresh = self._handle is None
        h = RectilinearGrid.handle.fget(self)
        if fresh:
            cell = np.asfortranarray(self._cell, dtype=np.uint8)
            try:
                _lib.check(_lib.lib().ocn_grid_set_immersed_boundary(h, cell.ctypes.data_as(C.POINTER(C.c_ubyte))))
            except Exception:
                _lib.lib().ocn_grid_destroy(h)
                self._handle = None
                raise
        return h

    def immersed_flags(self):
        """the two device tables of csrc/ocn_immersed.h as the library built them: (periphery bytes, orders words), parent-shaped at ccc"""
        P = tuple(n + 2 * h for n, h in zip(self.size, self.halo_size))
        periphery, orders = np.empty(P, dtype=np.uint8, order="F"), np.empty(P, dtype=np.uint16, order="F")
        _lib.check(_lib.lib().ocn_grid_get_immersed_flags(self.handle, periphery.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                          orders.ctypes.data_as(C.POINTER(C.c_ushort))))
        return periphery, orders

    def summary(self):
        names = "×".join(str(n) for n in self.size)
        return (f"{names} {NAME}{{Float64, {', '.join(t.__name__ for t in self.topology)}}} on {self.architecture} with "
                f"{self.halo_size} halo")

    def __repr__(self):
        return (f"{self.summary()}:\n├── immersed_boundary: {self.immersed_boundary.summary()}\n"
                f"└── underlying_grid: {RectilinearGrid.__repr__(self).replace(NAME, 'RectilinearGrid')}")


def mask_immersed_field(field, value=0.0):
    """mask_immersed_field!(field, value = 0) (mask_immersed_field.jl:24-64): field = value at immersed_peripheral_node of the field's
    location; nothing on a grid without a boundary (:46)"""
    if not isinstance(field.grid, ImmersedBoundaryGrid):
        return field
    if any(l is None for l in field.loc):
        refuse("mask_immersed_field! of a reduced field")
    _lib.check(_lib.lib().ocn_mask_immersed_field(field.grid.handle, field.data, _lib.i3(field.loc_codes), float(value)))
    return field


def validate_model(grid, closure, buoyancy_force, coriolis, background_fields, stokes_drift, particles, boundary_conditions):
    """what NonhydrostaticModel(grid = ibg, ...) refuses, before any handle exists"""
    from .boundary_conditions import scheme_sides
    from .buoyancy import ConstantCartesianCoriolis
    from .closures import AnisotropicMinimumDissipation, Smagorinsky, is_vertically_implicit
    if isinstance(closure, AnisotropicMinimumDissipation):
        refuse("AnisotropicMinimumDissipation (an eddy-viscosity closure)")
    if isinstance(closure, Smagorinsky):
        refuse("DynamicSmagorinsky (an eddy-viscosity closure)" if getattr(closure, "dynamic", False) else "Smagorinsky (an eddy-viscosity closure)")
    if is_vertically_implicit(closure):
        refuse("VerticallyImplicitTimeDiscretization")
    if buoyancy_force is not None and buoyancy_force.tilted:
        refuse("BuoyancyForce(gravity_unit_vector=...)")
    if isinstance(coriolis, ConstantCartesianCoriolis):
        refuse("ConstantCartesianCoriolis")
    if background_fields:
        refuse("background_fields")
    if stokes_drift is not None:
        refuse("stokes_drift")
    if particles is not None:
        refuse("particles (LagrangianParticles)")
    for fbcs in (boundary_conditions or {}).values():
        for tb in (fbcs.values() if isinstance(fbcs, dict) else [fbcs]):
            if scheme_sides(tb):
                refuse("an OpenBoundaryCondition with a scheme (PerturbationAdvection)")


FFT_WARNING = ("The FFT-based pressure_solver for NonhydrostaticModels on ImmersedBoundaryGrid\n"
               "is approximate and will probably produce velocity fields that are divergent\n"
               "adjacent to the immersed boundary. An experimental but improved pressure_solver\n"
               "(ConjugateGradientPoissonSolver) exists in the reference; it is not built here.")
