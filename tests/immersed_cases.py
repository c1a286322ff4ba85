"""The grids of the immersed-boundary tests (tests/test_immersed_host.py, tests/test_gpu_immersed.py): the smallest shapes on which every
cascade level, a stencil that sees the boundary from one side only, a boundary next to a wall and a periodic wrap of the mask occur.

  G1  (Periodic, Periodic, Bounded)  8 x 6 x 10  tanh-stretched z  halo (4, 4, 4)  GridFittedBottom bump
  G2  (Bounded, Bounded, Bounded)    7 x 6 x 8                      halo (4, 4, 4)  GridFittedBoundary: a 2 x 2 x 3 block on the west wall
                                                                                    plus one isolated cell
  G3  (Periodic, Flat, Bounded)      8 x 1 x 8                      halo (4, 4)     a step bottom
  G4  as G1                                                         halo (5, 4, 6)
  G5  (Periodic, Periodic, Periodic) 8 x 6 x 8                      halo (4, 4, 4)  GridFittedBoundary: a block in the middle and the two
                                                                                    cells in opposite corners, neighbours across every wrap
                                                                                    (the pressure step's source term reads wrapped indices)

The G1 bump, as the number of immersed cells per column: a row with none, columns of five, a one-cell-wide trench (column 3 between two
columns of five) and a column of three on the periodic edge whose neighbour across the wrap has none."""
import numpy as np

from helpers import tanh_faces

TOPO_CODE = {"Periodic": 0, "Bounded": 1, "Flat": 3}

_BUMP_X = np.array([0, 2, 5, 1, 5, 3, 0, 3])
_BUMP_Y = np.array([0, 0, 1, 3, 6, 1])
G1_CELLS = np.maximum(0, _BUMP_X[:, None] - _BUMP_Y[None, :])            # (8, 6): immersed cells per column


def _g1_bottom():
    zf = tanh_faces(10)
    return np.where(G1_CELLS > 0, zf[G1_CELLS], -2.0)                    # the face on top of the highest immersed cell; below the domain: none


def _g2_mask():
    mask = np.zeros((7, 6, 8), dtype=bool)
    mask[0:2, 2:4, 0:3] = True
    mask[4, 1, 5] = True
    return mask


def _g5_mask():
    mask = np.zeros((8, 6, 8), dtype=bool)
    mask[3:5, 2:4, 2:5] = True
    mask[0, 0, 0] = mask[7, 5, 7] = True
    return mask


CASES = {
    "G1": dict(topology=("Periodic", "Periodic", "Bounded"), size=(8, 6, 10), stretched=True, halo=(4, 4, 4), boundary=dict(bottom=_g1_bottom())),
    "G2": dict(topology=("Bounded", "Bounded", "Bounded"), size=(7, 6, 8), stretched=False, halo=(4, 4, 4), boundary=dict(mask=_g2_mask())),
    "G3": dict(topology=("Periodic", "Flat", "Bounded"), size=(8, 1, 8), stretched=False, halo=(4, 0, 4),
               boundary=dict(bottom=np.where(np.arange(8) >= 3, -0.6, -2.0).reshape(8, 1))),
    "G4": dict(topology=("Periodic", "Periodic", "Bounded"), size=(8, 6, 10), stretched=True, halo=(5, 4, 6), boundary=dict(bottom=_g1_bottom())),
    "G5": dict(topology=("Periodic", "Periodic", "Periodic"), size=(8, 6, 8), stretched=False, halo=(4, 4, 4), boundary=dict(mask=_g5_mask())),
}
EMPTY = dict(bottom=-2.0)            # a bottom below the domain: no immersed cell


def z_of(case):
    c = CASES[case]
    return tanh_faces(c["size"][2]) if c["stretched"] else (-1.0, 0.0)


def underlying_grid(ocn, arch, case, halo=None):
    c = CASES[case]
    flat = [t == "Flat" for t in c["topology"]]
    halo = c["halo"] if halo is None else halo
    kw = dict(size=tuple(n for n, f in zip(c["size"], flat) if not f), halo=tuple(h for h, f in zip(halo, flat) if not f),
              topology=tuple(getattr(ocn, t) for t in c["topology"]), z=z_of(case))
    if not flat[0]:
        kw["x"] = (0.0, 1.0)
    if not flat[1]:
        kw["y"] = (0.0, 1.0)
    return ocn.RectilinearGrid(arch, **kw)


def boundary_of(ocn, description):
    if "mask" in description:
        return ocn.GridFittedBoundary(description["mask"])
    condition = ocn.InterfaceImmersedCondition() if description.get("interface") else ocn.CenterImmersedCondition()
    return ocn.GridFittedBottom(description["bottom"], condition)


def immersed_grid(ocn, arch, case, boundary=None, halo=None):
    description = CASES[case]["boundary"] if boundary is None else boundary
    return ocn.ImmersedBoundaryGrid(underlying_grid(ocn, arch, case, halo), boundary_of(ocn, description))


def oracle_grid(oracle, case, halo=None):
    c = CASES[case]
    return oracle.Grid(c["size"], halo=c["halo"] if halo is None else halo, topology=tuple(TOPO_CODE[t] for t in c["topology"]),
                       x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(case))
