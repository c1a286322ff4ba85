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
columns of five) and a column of three on the periodic edge whose neighbour across the wrap has none.

TILE_CASES, a table of its own (the parametrisations over CASES assert what belongs to those five small grids): sizes around the 64 x 7
tiles of the flux-sharing tendency kernel (role_march, csrc/ocn_tendency_roles.h), whose eighth wave computes the y-fluxes of row j0 + 7
and the x-fluxes of column i0 + 64 of a tile. All (Periodic, Periodic, .), halo (4, 4, 4):

  T1   65 x  8 x 6  Bounded, tanh  GridFittedBottom    one column in the second x tile, one row in the second row tile: the edge wave is
                                                       live in x and in y
  T2  129 x 15 x 5  Bounded, tanh  GridFittedBottom    three x tiles, three row tiles (7 + 7 + 1)
  T3   64 x  7 x 7  Periodic       GridFittedBoundary  exactly one tile: both edge lines are the periodic wrap, their flags halo entries
  T4   63 x 14 x 4  Bounded        GridFittedBottom    one lane short of a tile, two whole row tiles
  T5  130 x  6 x 9  Periodic       GridFittedBoundary  a ragged third x tile, fewer rows than a tile
  T6  200 x  4 x 5  Bounded        GridFittedBottom    four x tiles, Ny at the halo's minimum

Each starts from a seeded draw (immersed cells per column, or a mask) and then places cells at the tile seams -- the faces i = 65, 129,
193 and j = 8, 15 that exist, and the periodic wrap N | 1 -- by hand: across every seam an immersed cell faces a fluid one in both
orientations (rows 2 and 3 for the x seams, columns 10 and 20 for the y seams, the orientation alternating from seam to seam so that a cell
two seams share gets one value), at every seam corner an immersed cell has a fluid diagonal neighbour, and column (31, 2) has no immersed
cell. tests/test_immersed_host.py::test_tile_cases_hold_what_they_promise asserts from the restatement's tables what that gives."""
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

X_SEAMS, Y_SEAMS = (65, 129, 193), (8, 15)          # the first face of a second, third, fourth tile of 64 columns / 7 rows


def seams(n, faces):
    """(the cell before the seam, the seam cell) of every tile seam along a direction of n cells: the faces that exist, then the wrap"""
    return [(s - 1, s) for s in faces if s <= n] + [(n, 1)]


def seam_corners(size):
    """(seam column, seam row) pairs the hand-placed corners sit at: the q-th x seam with the q-th y seam -- without the corner of the two
    wraps where there is another: its diagonal neighbour, cell (Nx, Ny), is the corner cell (65, 8) of T1 and (129, 15) of T2"""
    corners = [(x[1], y[1]) for x, y in zip(seams(size[0], X_SEAMS), seams(size[1], Y_SEAMS))]
    return corners[:-1] if len(corners) > 1 and corners[-1] == (1, 1) else corners


def _tile_cells(size, seed):
    """immersed cells per column of a GridFittedBottom tile case: a thinned seeded draw of 0 .. Nz - 1, then the seams"""
    Nx, Ny, Nz = size
    rng = np.random.default_rng(seed)
    n = np.where(rng.random((Nx, Ny)) < 0.35, rng.integers(1, Nz, (Nx, Ny)), 0)
    high, low = Nz - 1, max(1, Nz // 2)
    for q, (a, b) in enumerate(seams(Nx, X_SEAMS)):
        a, b = ((a, b), (b, a))[q % 2]
        n[a - 1, 1], n[b - 1, 1] = high, 0            # row 2
        n[a - 1, 2], n[b - 1, 2] = 0, low             # row 3
    for q, (a, b) in enumerate(seams(Ny, Y_SEAMS)):
        a, b = ((a, b), (b, a))[q % 2]
        n[9, a - 1], n[9, b - 1] = high, 0            # column 10
        n[19, a - 1], n[19, b - 1] = 0, low           # column 20
    for i, j in seam_corners(size):
        n[i - 1, j - 1], n[(i - 2) % Nx, (j - 2) % Ny] = 2, 0
    n[30, 1] = 0
    return n


def _tile_bottom(size, seed, stretched):
    n = _tile_cells(size, seed)
    zf = tanh_faces(size[2]) if stretched else np.linspace(-1.0, 0.0, size[2] + 1)
    return np.where(n > 0, zf[n], -2.0)


def _tile_mask(size, seed):
    """the mask of a GridFittedBoundary tile case (Nz >= 7): a seeded draw of one cell in ten, then the seams at levels 2 and 3 (level 5 of
    the same rows and columns left fluid on both sides), the corners at level 4"""
    Nx, Ny, Nz = size
    mask = np.random.default_rng(seed).random(size) < 0.1
    for q, (a, b) in enumerate(seams(Nx, X_SEAMS)):
        mask[a - 1, 1, 4] = mask[b - 1, 1, 4] = False
        a, b = ((a, b), (b, a))[q % 2]
        mask[a - 1, 1, 1], mask[b - 1, 1, 1] = True, False
        mask[a - 1, 2, 2], mask[b - 1, 2, 2] = False, True
    for q, (a, b) in enumerate(seams(Ny, Y_SEAMS)):
        mask[9, a - 1, 4] = mask[9, b - 1, 4] = False
        a, b = ((a, b), (b, a))[q % 2]
        mask[9, a - 1, 1], mask[9, b - 1, 1] = True, False
        mask[19, a - 1, 2], mask[19, b - 1, 2] = False, True
    for i, j in seam_corners(size):
        mask[i - 1, j - 1, 3], mask[(i - 2) % Nx, (j - 2) % Ny, 3] = True, False
    mask[30, 1, :] = False
    return mask


def _tile_case(size, seed, z):
    """z: "tanh" | "bounded" (GridFittedBottom) | "periodic" (GridFittedBoundary)"""
    boundary = dict(mask=_tile_mask(size, seed)) if z == "periodic" else dict(bottom=_tile_bottom(size, seed, z == "tanh"))
    return dict(topology=("Periodic", "Periodic", "Periodic" if z == "periodic" else "Bounded"), size=size, stretched=z == "tanh", halo=(4, 4, 4),
                boundary=boundary)


TILE_CASES = {
    "T1": _tile_case((65, 8, 6), 101, "tanh"),
    "T2": _tile_case((129, 15, 5), 102, "tanh"),
    "T3": _tile_case((64, 7, 7), 103, "periodic"),
    "T4": _tile_case((63, 14, 4), 104, "bounded"),
    "T5": _tile_case((130, 6, 9), 105, "periodic"),
    "T6": _tile_case((200, 4, 5), 106, "bounded"),
}


def case_of(case):
    return CASES[case] if case in CASES else TILE_CASES[case]


def empty_boundary(case):
    """a boundary without an immersed cell: the bottom below the domain, or -- Periodic z, where the halo levels under such a bottom would
    be immersed -- a mask of zeros"""
    c = case_of(case)
    return dict(mask=np.zeros(c["size"], dtype=bool)) if c["topology"][2] == "Periodic" else EMPTY


def z_of(case):
    c = case_of(case)
    return tanh_faces(c["size"][2]) if c["stretched"] else (-1.0, 0.0)


def underlying_grid(ocn, arch, case, halo=None):
    c = case_of(case)
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
    description = case_of(case)["boundary"] if boundary is None else boundary
    return ocn.ImmersedBoundaryGrid(underlying_grid(ocn, arch, case, halo), boundary_of(ocn, description))


def oracle_grid(oracle, case, halo=None):
    c = case_of(case)
    return oracle.Grid(c["size"], halo=c["halo"] if halo is None else halo, topology=tuple(TOPO_CODE[t] for t in c["topology"]),
                       x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(case))
