"""Halo sizes other than (3, 3, 3): the cases of tests/test_halo_sizes_host.py and tests/test_gpu_halo_sizes.py. Plain data and
slicing helpers, no fixtures.

HALOS: the three asymmetric tuples give every direction each of three distinct values (x: 5, 3, 4; y: 3, 4, 6; z: 4, 6, 3), so Hx, Hy,
Hz used in each other's place -- or a literal 3 where a halo was meant -- shows in at least two of them; (7, 7, 7) gives H <= N < 2H on
the small grids below: both sides' periodic images overlap, and the halo strips are wider than the 3-row tiles.
Every grid keeps N >= H in every direction (grids.py refuses anything else)."""
import numpy as np

from helpers import tanh_faces

BASE = (3, 3, 3)
HALOS = ((5, 3, 4), (3, 4, 6), (4, 6, 3), (7, 7, 7))

PPP = ("Periodic", "Periodic", "Periodic")
PPB = ("Periodic", "Periodic", "Bounded")
BBB = ("Bounded", "Bounded", "Bounded")
BPB = ("Bounded", "Periodic", "Bounded")
PFB = ("Periodic", "Flat", "Bounded")
ALL_TOPOLOGIES = [(a, b, c) for a in ("Periodic", "Bounded") for b in ("Periodic", "Bounded") for c in ("Periodic", "Bounded")]

# name -> (topology, size, stretched z). The two tendency grids are those of test_gpu_option_variants.py: two ragged x tiles
# (70 = 64 + 6, 66 = 64 + 2), two y tiles, several z chunks
GRIDS = {
    "ppp": (PPP, (70, 12, 20), False),
    "ppb": (PPB, (66, 9, 14), True),
    "bbb": (BBB, (12, 10, 8), False),
    "pfb": (PFB, (16, 1, 8), True),
}
FILL_SIZES = ((8, 8, 8), (16, 9, 7))
# the oracle-invariance cases of the host file
ORACLE_CASES = {
    "ppp": (PPP, (12, 10, 8), False, None),
    "ppb_physics": (PPB, (12, 10, 8), True, "amd"),
    "bbb_scalar": (BBB, (9, 8, 7), False, "scalar"),
    "bpb": (BPB, (12, 10, 8), True, None),
}
ORACLE_TOPO = {"Periodic": 0, "Bounded": 1, "Flat": 3}


def clamped(halo, size):
    """the halo with every entry cut to its direction's size: where a grid of a case is shorter than the halo asked for, it takes the deepest
    halo it admits (N == H there)"""
    return tuple(min(h, n) for h, n in zip(halo, size))


class AtHalo:
    """the package, or the oracle module, with another default halo: grids built without a `halo` keyword get `halo` (clamped to the grid's
    size; an explicit `halo` is kept). Everything else is the wrapped module's. It lets the halo-general helpers of the feature tests -- they
    build their grids through the module handed to them -- run at another halo."""

    def __init__(self, module, halo):
        self.__dict__["_module"], self.__dict__["_halo"] = module, tuple(halo)

    def __getattr__(self, name):
        return getattr(self._module, name)

    def RectilinearGrid(self, architecture, size, **kw):
        if kw.get("halo") is None:
            topology = kw.get("topology", (self._module.Periodic,) * 3)
            flat = [(t if isinstance(t, type) else type(t)) is self._module.Flat for t in topology]
            size_t = tuple(size) if isinstance(size, (tuple, list)) else (size,)
            it = iter(size_t)
            full = size_t if len(size_t) == 3 else tuple(1 if f else next(it) for f in flat)
            kw["halo"] = tuple(0 if f else h for h, f in zip(clamped(self._halo, full), flat))
        return self._module.RectilinearGrid(architecture, size=size, **kw)

    def Grid(self, size, halo=None, **kw):
        return self._module.Grid(size, halo=clamped(self._halo, size) if halo is None else halo, **kw)


def halo_id(h):
    return "H%d%d%d" % tuple(h)


def zcoord(topology, size, stretched):
    if stretched:
        return tanh_faces(size[2])
    return (-1.0, 0.0) if topology[2] == "Bounded" else (0.0, 1.0)


def make_grid(ocn, arch, topology, size, halo, stretched=False):
    """the product's grid (arch = None: host metadata only)"""
    flat = [t == "Flat" for t in topology]
    halo = tuple(0 if f else h for h, f in zip(halo, flat))
    return ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=zcoord(topology, size, stretched),
                               topology=tuple(getattr(ocn, t) for t in topology), halo=halo)


def make_oracle_grid(O, topology, size, halo, stretched=False):
    return O.Grid(size, halo=halo, topology=tuple(ORACLE_TOPO[t] for t in topology), x=(0.0, 1.0), y=(0.0, 1.0),
                  z=zcoord(topology, size, stretched))


def face_code(ocn, loc):
    """(Face, Center, Center) -> (1, 0, 0): the oracle's location code"""
    return tuple(1 if l is ocn.Face else 0 for l in loc)


def interior(grid, a, loc=None):
    """the interior of a parent array, from the grid's OWN halo and the field's location. grid: the product's RectilinearGrid or the
    oracle's Grid; loc: Face / Center classes, 0 / 1 codes, or None for the cell interior (Nx, Ny, Nz) whatever the location"""
    if hasattr(grid, "halo_size"):
        H, N = grid.halo_size, grid.size
        wall = [t.__name__ in ("Bounded", "LeftConnected") for t in grid.topology]
    else:
        H, N = grid.H, grid.N
        wall = [t == 1 for t in grid.topo]
    sl = []
    for d in range(3):
        face = loc is not None and (loc[d] == 1 or getattr(loc[d], "__name__", "") == "Face")
        sl.append(slice(H[d], H[d] + N[d] + (1 if (face and wall[d]) else 0)))
    return a[tuple(sl)]


def periodic_pad(grid, core):
    """the cell interior padded periodically by the grid's halo in every direction (whole parent array of a triply periodic field)"""
    return np.pad(core, [(h, h) for h in grid.halo_size], mode="wrap")
