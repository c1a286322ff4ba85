"""CPU: ImmersedBoundaryGrid on the host, and what tests/test_gpu_immersed.py rests on.

  * the reference's data-free grid tests (test/test_immersed_boundary_grid.jl): bottom heights snapped to faces (:131-152), cell detection
    z <= z_b (:88-108), function and array GridFittedBoundary (:222-282), Flat topologies (:328-356), equality (:389-453); number, array
    and function bottoms on a stretched z; InterfaceImmersedCondition against the loop of grid_fitted_bottom.jl:111-122;
  * the numpy restatement (tests/immersed_reference.py) with an empty boundary == background_reference.advective_tendency == the oracle,
    bit for bit, on G1, G2, G3 and at the tile-edge sizes T1 and T3; its predicates on a hand-checked configuration; what the tile-edge
    cases hold at every tile seam; one finite step of ImmersedOrchestrated on every grid;
  * halo inflation to buffer + 1 with the reference's warning text; every refusal; the new symbols of the built library.

No GPU."""
import ctypes as C
import warnings

import numpy as np
import pytest

import background_reference as B
import immersed_cases as IC
import immersed_reference as IR
import vertically_implicit_reference as R
from helpers import smooth_state, tanh_faces


@pytest.fixture(scope="module")
def ocn():
    import oldoceananigans_jl_amd as ocn
    return ocn


def _ppb(ocn, size, **kw):
    return ocn.RectilinearGrid(None, size=size, topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's grid tests
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_fitted_bottom_cell_detection(ocn):
    """test_immersed_boundary_grid.jl:88-108: 4 x 4 x 8, extent 1, z_b = -0.5: a cell is immersed when z_centre <= z_b"""
    ibg = ocn.ImmersedBoundaryGrid(_ppb(ocn, (4, 4, 8), extent=(1, 1, 1)), ocn.GridFittedBottom(-0.5))
    cell = ibg.immersed_cell_mask()
    H = ibg.halo_size
    zc = ibg.nodes((ocn.Center,) * 3)[2].ravel()
    for i in range(4):
        for j in range(4):
            for k in range(8):
                assert cell[i + H[0], j + H[1], k + H[2]] == (zc[k] <= -0.5)
    assert cell.shape == ibg.total_size((ocn.Center,) * 3) and cell.dtype == bool
    assert cell[:, :, :H[2]].all() and not cell[:, :, H[2] + 8:].any()               # halos: below the bottom, above the surface


def test_bottom_height_is_snapped_to_faces(ocn):
    """:131-152: 6 x 6 x 8, a function bottom: every numerical bottom height is a z face"""
    bottom = lambda x, y: -0.25 + 0.1 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)          # noqa: E731
    ibg = ocn.ImmersedBoundaryGrid(_ppb(ocn, (6, 6, 8), extent=(1, 1, 1)), ocn.GridFittedBottom(bottom))
    zb = ibg.immersed_boundary.bottom_height.interior()
    zfaces = ibg.nodes((ocn.Center, ocn.Center, ocn.Face))[2].ravel()
    assert zb.shape == (6, 6, 1) and np.isin(zb, zfaces).all()
    assert len(np.unique(zb)) > 1
    # halos of the bottom: the Periodic copy
    parent, H = ibg.immersed_boundary.bottom_height.parent(), ibg.halo_size
    assert np.array_equal(parent[:H[0], H[1]:-H[1]], parent[6:6 + H[0], H[1]:-H[1]])


def test_grid_fitted_boundary_function_and_array(ocn):
    """:222-282"""
    grid = _ppb(ocn, (4, 4, 4), extent=(2, 2, 1))
    mask_function = lambda x, y, z: x ** 2 + y ** 2 + z ** 2 <= 0.25                            # noqa: E731
    ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBoundary(mask_function))
    assert ibg.architecture is grid.architecture and ibg.size == grid.size and ibg.halo_size == grid.halo_size and ibg.topology == grid.topology
    assert ibg.immersed_boundary.mask.parent().dtype == bool
    x, y, z = ibg.nodes((ocn.Center,) * 3)
    assert np.array_equal(ibg.immersed_boundary.mask.interior(), np.broadcast_to(mask_function(x, y, z), (4, 4, 4)))
    assert ibg.immersed_boundary.mask.interior().any()
    grid = _ppb(ocn, (3, 3, 3), extent=(1, 1, 1))
    mask = np.zeros((3, 3, 3), dtype=bool)
    mask[1, 1, 1] = True
    ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBoundary(mask))
    cell, H = ibg.immersed_cell_mask(), ibg.halo_size
    assert cell[1 + H[0], 1 + H[1], 1 + H[2]] and not cell[H[0], H[1], H[2]] and not cell[2 + H[0], 2 + H[1], 2 + H[2]]
    assert ibg.size == grid.size


def test_flat_topologies(ocn):
    """:328-356"""
    for topo, size, extent in (((ocn.Flat, ocn.Periodic, ocn.Bounded), (5, 5), (1, 1)), ((ocn.Periodic, ocn.Flat, ocn.Bounded), (5, 5), (1, 1)),
                               ((ocn.Flat, ocn.Flat, ocn.Bounded), 5, 1)):
        grid = ocn.RectilinearGrid(None, topology=topo, size=size, extent=extent)
        ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBottom(-0.3))
        assert ibg.topology == topo and ibg.architecture is None
        cell = ibg.immersed_cell_mask()
        assert cell.shape == ibg.total_size((ocn.Center,) * 3)
        zc = ibg.nodes((ocn.Center,) * 3)[2].ravel()
        assert np.array_equal(ibg.underlying_grid.nodes((ocn.Center,) * 3)[2].ravel(), zc)
        column = cell[(0 if topo[0] is ocn.Flat else ibg.Hx), (0 if topo[1] is ocn.Flat else ibg.Hy), ibg.Hz:ibg.Hz + 5]
        assert np.array_equal(column, zc <= -0.3) and column.any() and not column.all()


def test_equality(ocn):
    """:389-453 (the PartialCellBottom arms apart: that boundary is refused)"""
    assert ocn.GridFittedBottom(1) == ocn.GridFittedBottom(1) and ocn.GridFittedBottom(1) != ocn.GridFittedBottom(2)
    f = lambda x, y: 0.2 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)                        # noqa: E731
    assert ocn.GridFittedBottom(f) == ocn.GridFittedBottom(f)
    assert ocn.GridFittedBottom(f) != ocn.GridFittedBottom(f, ocn.InterfaceImmersedCondition())
    m1 = lambda x, y, z: x ** 2 + y ** 2 + z ** 2 <= 0.25                                       # noqa: E731
    m3 = lambda x, y, z: x ** 2 + y ** 2 + z ** 2 <= 0.5                                        # noqa: E731
    assert ocn.GridFittedBoundary(m1) == ocn.GridFittedBoundary(m1) and ocn.GridFittedBoundary(m1) != ocn.GridFittedBoundary(m3)
    assert ocn.GridFittedBoundary(m1) != ocn.GridFittedBottom(1)
    a1, a2, a3 = (np.zeros((3, 3, 3), dtype=bool) for _ in range(3))
    a1[1, 1, 1] = a2[1, 1, 1] = a3[0, 0, 0] = True
    assert ocn.GridFittedBoundary(a1) == ocn.GridFittedBoundary(a2) and ocn.GridFittedBoundary(a1) != ocn.GridFittedBoundary(a3)
    assert ocn.GridFittedBoundary(a1) != ocn.GridFittedBoundary(m1)


@pytest.mark.parametrize("interface", [False, True], ids=["center", "interface"])
def test_bottoms_on_a_stretched_z_against_the_loop(ocn, interface):
    """number, array and function bottoms on a tanh-stretched z, CenterImmersedCondition and InterfaceImmersedCondition: the numerical
    bottom height and the cell mask == the loop of grid_fitted_bottom.jl:111-122 restated in tests/immersed_reference.py"""
    grid = _ppb(ocn, (5, 4, 9), x=(0.0, 1.0), y=(0.0, 2.0), z=tanh_faces(9), halo=(4, 4, 4))
    condition = ocn.InterfaceImmersedCondition() if interface else ocn.CenterImmersedCondition()
    array = -0.9 + 0.8 * np.random.default_rng(3).uniform(size=(5, 4))
    function = lambda x, y: -0.5 + 0.3 * np.sin(2 * np.pi * x) + 0.05 * y                       # noqa: E731
    seen = set()
    for bottom in (-0.37, float(tanh_faces(9)[4]), array, function):
        ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBottom(bottom, condition))
        cell, num = IR.cells_of_grid(grid, dict(bottom=bottom, interface=interface))
        assert np.array_equal(ibg.immersed_cell_mask(), cell)
        assert np.array_equal(ibg.immersed_boundary.bottom_height.parent()[:, :, 0], num)
        seen.add(int(cell[4:-4, 4:-4, 4:-4].sum()))
        assert "GridFittedBottom(" in ibg.immersed_boundary.summary() and "ImmersedBoundaryGrid{Float64, Periodic, Periodic, Bounded}" in repr(ibg)
    assert len(seen) > 1
    # a bottom exactly on a face: the cell below it is immersed either way, the one above only if its centre were below
    zf = tanh_faces(9)
    ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBottom(float(zf[4]), condition))
    assert ibg.immersed_cell_mask()[6, 6, 4:4 + 9].sum() == 4
    # a bottom between a centre and the face above it: Center immerses the cell, Interface snaps to the face below
    zc = 0.5 * (zf[3] + zf[4])
    ibg = ocn.ImmersedBoundaryGrid(grid, ocn.GridFittedBottom(0.5 * (zc + zf[4]), condition))
    assert ibg.immersed_boundary.bottom_height.interior()[0, 0, 0] == (zf[3] if interface else zf[4])


def test_cases_hold_what_they_promise():
    """G1: a column without immersed cells, one with >= 4, a one-cell-wide trench, a boundary across the periodic wrap"""
    n = IC.G1_CELLS
    assert (n == 0).any() and (n >= 4).any() and n[3, 0] < n[2, 0] - 3 and n[3, 0] < n[4, 0] - 3 and n[7, 0] > 0 and n[0, 0] == 0


@pytest.mark.parametrize("case", list(IC.TILE_CASES))
def test_tile_cases_hold_what_they_promise(ocn, case):
    """the tile-edge cases, from the restatement's tables. At every x seam (the faces i = 65, 129, 193 that exist and the wrap Nx | 1): an
    immersed cell faces a fluid one across it, in both orientations over the case's seams; both x order entries fall below 3 at the seam
    column and at the column before it; IMM_FCC of the seam face is set at one level of a row and clear at another. The same at every y
    seam (j = 8, 15, the wrap) with the y entries and IMM_CFC. At every corner the case places, an immersed cell has a fluid diagonal
    neighbour and IMM_FFC is set. The flags the edge wave reads beyond the periodic edge (column Nx + 1, row Ny + 1) are those of column /
    row 1. Elsewhere: a column without an immersed cell, and every cascade level the grid admits along z on both sides -- {1, 2, 3} on a
    Periodic z; next to the walls of a Bounded z the window of buffer 3 is free only for 4 <= k <= Nz - 2 (side ᶠ) / 3 <= k <= Nz - 2
    (side ᶜ) (test_predicates_by_hand), so level 3 needs Nz >= 6 / Nz >= 5 and T2, T4, T6 (Nz = 5, 4, 5) cannot hold it on every side."""
    grid, cells = _cells(ocn, case)
    imm = IR.Immersed(R.Metrics.of_grid(grid), cells)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = imm.m.N, imm.m.H
    at = lambda table, i, j, k: table[i - 1 + Hx, j - 1 + Hy, k - 1 + Hz]                       # noqa: E731   1-based, halos in reach
    cell = lambda i, j, k: at(imm.cell, i, j, k)                                                # noqa: E731
    bit = lambda loc, i, j, k: ((at(imm.periphery, i, j, k) >> IR.BIT[loc]) & 1).astype(bool)   # noqa: E731
    order = lambda d, side, i, j, k: (at(imm.orders, i, j, k) >> (2 * (2 * d + side))) & 3      # noqa: E731
    I, J, K = np.arange(1, Nx + 1), np.arange(1, Ny + 1), np.arange(1, Nz + 1)
    fcc, cfc, ffc = (R.FACE, R.CENTER, R.CENTER), (R.CENTER, R.FACE, R.CENTER), (R.FACE, R.FACE, R.CENTER)

    def seam(d, before, on, loc):
        """-> the orientations met across the seam between the lines `before` and `on` along direction d"""
        line = (lambda n: (n, J[:, None], K[None, :])) if d == 0 else (lambda n: (I[:, None], n, K[None, :]))     # noqa: E731
        solid_before, solid_on = cell(*line(before)), cell(*line(on))
        met = {name for name, there in (("solid|fluid", solid_before & ~solid_on), ("fluid|solid", ~solid_before & solid_on)) if there.any()}
        assert met, (d, on)
        for n in (before, on):
            for side in (0, 1):
                assert (order(d, side, *line(n)) < 3).any(), (d, n, side)
        flag = bit(loc, *line(on))
        assert (flag.any(axis=1) & ~flag.all(axis=1)).any(), (d, on)
        return met

    x_seams, y_seams = IC.seams(Nx, IC.X_SEAMS), IC.seams(Ny, IC.Y_SEAMS)
    assert [s[1] for s in x_seams] == [i for i in (65, 129, 193) if i <= Nx] + [1] and x_seams[-1][0] == Nx
    assert [s[1] for s in y_seams] == [j for j in (8, 15) if j <= Ny] + [1] and y_seams[-1][0] == Ny
    assert set().union(*(seam(0, a, b, fcc) for a, b in x_seams)) == {"solid|fluid", "fluid|solid"}
    assert set().union(*(seam(1, a, b, cfc) for a, b in y_seams)) == {"solid|fluid", "fluid|solid"}
    corners = IC.seam_corners((Nx, Ny, Nz))
    assert corners and (Nx < 65 or corners[0][0] == 65)                                         # where it is live, the edge wave's column
    for i, j in corners:
        assert (cell(i, j, K) & ~cell(i - 1, j - 1, K) & bit(ffc, i, j, K)).any(), (i, j)
    for table in (imm.periphery, imm.orders):
        assert np.array_equal(at(table, Nx + 1, J[:, None], K[None, :]), at(table, 1, J[:, None], K[None, :]))
        assert np.array_equal(at(table, I[:, None], Ny + 1, K[None, :]), at(table, I[:, None], 1, K[None, :]))
    inside = cell(I[:, None, None], J[None, :, None], K[None, None, :])
    assert (~inside.any(axis=2)).any() and inside.any()
    periodic = IC.TILE_CASES[case]["topology"][2] == "Periodic"
    for side, first in ((0, 4), (1, 3)):
        levels = set(np.unique(order(2, side, I[:, None, None], J[None, :, None], K[None, None, :])))
        assert levels == ({1, 2, 3} if periodic or first <= Nz - 2 else {1, 2}), (side, levels)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _cells(ocn, case, boundary=None):
    grid = IC.underlying_grid(ocn, None, case)
    return grid, IR.cells_of_grid(grid, IC.case_of(case)["boundary"] if boundary is None else boundary)[0]


@pytest.mark.parametrize("case", list(IC.CASES) + list(IC.TILE_CASES))
def test_package_mask_is_the_restatement(ocn, case):
    grid, cell = _cells(ocn, case)
    ibg = IC.immersed_grid(ocn, None, case)
    assert np.array_equal(ibg.immersed_cell_mask(), cell) and cell[tuple(slice(h, s - h) for h, s in zip(grid.halo_size, cell.shape))].any()


def test_predicates_by_hand(ocn):
    """the configuration drawn in immersed_boundary_interface.jl:22-47 (cell i - 1 immersed, cell i fluid) on G2, and the wall cases: a
    node on the domain's wall is peripheral for the underlying grid and therefore NOT an immersed peripheral node"""
    grid, cell = _cells(ocn, "G2")
    imm = IR.Immersed(R.Metrics.of_grid(grid), cell)
    one = lambda v: bool(np.asarray(v).reshape(-1)[0])                                          # noqa: E731
    A = lambda *ijk: tuple(np.array([[[x]]]) for x in ijk)                                      # noqa: E731
    fcc, ccc = (R.FACE, R.CENTER, R.CENTER), (R.CENTER,) * 3
    # the block covers i = 1..2, j = 3..4, k = 1..3: i = 3 is the fluid cell next to it
    assert not one(imm.inactive_node(*A(3, 3, 1), fcc)) and not one(imm.inactive_node(*A(3, 3, 1), ccc))
    assert one(imm.inactive_node(*A(2, 3, 1), ccc)) and one(imm.inactive_node(*A(2, 3, 1), fcc))
    assert one(imm.immersed_peripheral_node(*A(3, 3, 1), fcc)) and not one(imm.immersed_peripheral_node(*A(4, 3, 1), fcc))
    # the face on the west wall belongs to the underlying periphery
    assert one(imm.peripheral_node(*A(1, 3, 1), fcc)) and not one(imm.immersed_peripheral_node(*A(1, 3, 1), fcc))
    # the isolated cell (5, 2, 6): all six faces around it are immersed peripheral nodes, the cell itself too
    for loc, ijk in ((fcc, (5, 2, 6)), (fcc, (6, 2, 6)), ((R.CENTER, R.FACE, R.CENTER), (5, 3, 6)), ((R.CENTER, R.CENTER, R.FACE), (5, 2, 7)), (ccc, (5, 2, 6))):
        assert one(imm.immersed_peripheral_node(*A(*ijk), loc))
    # the orders next to it along x, side ᶠ (windows of cells i - b .. i + b - 1): faces 5 and 6 touch it with b = 1, faces 4 and 7 reach it
    # with b = 2 (cells 2..5, 5..8), face 8 is the east wall (Nx = 7), face 3 reaches the west wall with b = 3 (cells 0..5)
    for i, want in ((5, 1), (6, 1), (7, 1), (8, 1)):
        assert int(imm.order(0, False, *A(i, 2, 6)).reshape(-1)[0]) == want, i
    assert int(imm.order(0, False, *A(4, 2, 6)).reshape(-1)[0]) == 1 and int(imm.order(0, False, *A(3, 2, 6)).reshape(-1)[0]) == 2
    # away from everything but the walls: the topological rule i >= b + 1, i <= N + 1 - b (row j = 6, level 8)
    got = [int(imm.order(0, False, *A(i, 6, 8)).reshape(-1)[0]) for i in range(1, 9)]
    assert got == [1, 1, 2, 3, 3, 2, 1, 1]
    got = [int(imm.order(0, True, *A(i, 6, 8)).reshape(-1)[0]) for i in range(0, 9)]         # side ᶜ: i >= b, i <= N + 1 - b
    assert got == [1, 1, 2, 3, 3, 3, 2, 1, 1]


@pytest.mark.parametrize("case", ["G1", "G2", "G3", "T1", "T3"])
def test_empty_boundary_is_the_plain_restatement_is_the_oracle(ocn, oracle, case):
    """with a bottom below the domain (T3, Periodic z: a mask of zeros) the immersed restatement's tendencies ==
    background_reference.advective_tendency == the oracle's compute_G, bit for bit: the order table reproduces outside_*_halo at the walls
    and no flux is masked. T1 (65 x 8 x 6) and T3 (64 x 7 x 7) pin the restatement at the tile-edge sizes tests/test_gpu_immersed.py uses."""
    g = IC.oracle_grid(oracle, case)
    m = R.Metrics.of_oracle(g)
    grid, cell = _cells(ocn, case, IC.empty_boundary(case))
    assert not cell[tuple(slice(h, s - h) for h, s in zip(m.H, cell.shape))].any()
    imm = IR.Immersed(m, cell)
    assert not (imm.periphery >> 1).any()
    rng = np.random.default_rng(11)
    P = {n: np.asfortranarray(rng.standard_normal(g.parent_size(R.LOCS[n]))) for n in "uvwc"}
    raw_w = P["w"].copy(order="F")
    for n in "uvwc":                                       # halo-filled fields: the wall-normal velocity vanishes on its walls
        g.fill_halo_regions(P[n], R.LOCS[n])
    adv = (P["u"], P["v"], P["w"])
    if case == "G1":
        # The one place the immersed methods part from the plain ones without an immersed cell: the advecting transport on
        # the HIGH wall face (k = Nz + 1) is interpolated across the wall-normal direction at a level whose cells are all inactive, so the
        # immersed cascade takes Centered(order = 2) where the plain one keeps order 4. An impenetrable wall has no transport there and both
        # give 0; with a w that does not vanish on the top wall the u tendency of the top level differs, and only that level.
        a = IR.advective_tendency(m, imm, "u", (P["u"], P["v"], raw_w), P["u"])
        b = B.advective_tendency(m, "u", (P["u"], P["v"], raw_w), P["u"])
        differs = np.argwhere(a != b)
        assert len(differs) and set(differs[:, 2]) == {m.N[2] - 1 + m.H[2]}
    for n in "uvwc":
        mine = IR.advective_tendency(m, imm, n, adv, P[n])
        plain = B.advective_tendency(m, n, adv, P[n])
        theirs = g.zeros(R.LOCS[n])
        g.compute_G(n, P["u"], P["v"], P["w"], theirs, c=P["c"] if n == "c" else None)
        assert np.array_equal(mine, plain) and np.array_equal(plain, theirs), n
        assert np.abs(mine).max() > 0
    # ... and the closure term and FPlane
    for n in "uvwc":
        G1_, G2_ = (np.asfortranarray(rng.standard_normal(P[n].shape)) for _ in range(2))
        G2_[...] = G1_
        IR.immersed_closure_part(m, imm, n, P, P[n], 3e-3, G1_)
        R.explicit_part(m, n, P, P[n], 3e-3, G2_)
        assert np.array_equal(G1_, G2_), n
    Gu, Gv = g.zeros(R.LOCS["u"]), g.zeros(R.LOCS["v"])
    Ou, Ov = g.zeros(R.LOCS["u"]), g.zeros(R.LOCS["v"])
    IR.fplane(m, imm, 0.7, P, Gu, Gv)
    oracle.lib().oro_add_fplane_coriolis(g.handle, 0.7, oracle._dp(P["u"]), oracle._dp(P["v"]), oracle._dp(Ou), oracle._dp(Ov))
    assert np.array_equal(Gu, Ou) and np.array_equal(Gv, Ov) and np.abs(Gu).max() > 0


@pytest.mark.parametrize("case", list(IC.CASES))
def test_orchestrated_takes_a_finite_step(ocn, oracle, case):
    """one RK3 and one AB2 step of ImmersedOrchestrated on every grid: finite, tracers exactly zero at their immersed nodes after
    update_state, the immersed boundary felt (the result differs from the empty boundary's)"""
    g = IC.oracle_grid(oracle, case)
    grid = IC.underlying_grid(ocn, None, case)
    results = []
    for boundary in (None, IC.EMPTY):
        cell = _cells(ocn, case, boundary)[1]
        yard = IR.ImmersedOrchestrated(oracle, g, 1, 2e-3, (1e-3,), cell, buoyancy_index=0, fcor=0.5)
        locs = {"u": (ocn.Face, ocn.Center, ocn.Center), "v": (ocn.Center, ocn.Face, ocn.Center), "w": (ocn.Center, ocn.Center, ocn.Face),
                "T": (ocn.Center,) * 3}
        vals = smooth_state({n: grid.nodes(l) for n, l in locs.items()}, 5)
        yard.set(u=vals["u"], v=vals["v"], w=vals["w"], c0=vals["T"])
        yard.time_step(0.05 / grid.Nx)
        yard.time_step_ab2(0.05 / grid.Nx)
        assert all(np.isfinite(a).all() for a in yard.U.values()) and np.isfinite(yard.p).all()
        results.append(yard)
    yard, empty = results
    inside = tuple(slice(h, h + n) for h, n in zip(yard.m.H, yard.m.N))
    assert np.all(yard.U["c0"][inside][yard.imm.cell[inside]] == 0.0)
    assert not np.array_equal(yard.U["u"], empty.U["u"])


# ---------------------------------------------------------------------------------------------------------------------
# the model's host side
# ---------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _no_handle(monkeypatch, ocn):
    def stop(self, grid, ntracers):
        raise _Stop(grid)
    monkeypatch.setattr(ocn.NonhydrostaticModel, "_create_handle", stop)


def test_halo_inflation_and_warnings(ocn, monkeypatch):
    """inflate_halo_size_one_dimension(req, old, _, ::IBG) = max(req + 1, old): halo 4 in every non-Flat direction for WENO(order = 5); the
    grid is recreated, the boundary materialised again, with the reference's warning (nonhydrostatic_model.jl:252-256) and the warning
    that the FFT-based solver is approximate (NonhydrostaticModels.jl:42-58)"""
    _no_handle(monkeypatch, ocn)
    ibg = IC.immersed_grid(ocn, None, "G3", halo=(3, 0, 3))
    assert ocn.inflate_halo_size(*ibg.halo_size, ibg, ocn.WENO()) == (4, 0, 4)
    assert ocn.inflate_halo_size(5, 0, 6, ibg, ocn.WENO()) == (5, 0, 6)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(_Stop) as stop:
            ocn.NonhydrostaticModel(grid=ibg, tracers=("b",))
    text = [str(w.message) for w in caught]
    assert sum("Inflating model grid halo size to (4, 0, 4) and recreating grid." in t and
               "an ImmersedBoundaryGrid requires an extra halo point in all non-flat directions" in t for t in text) == 1
    assert sum("The FFT-based pressure_solver for NonhydrostaticModels on ImmersedBoundaryGrid" in t and "approximate" in t for t in text) == 1
    new = stop.value.args[0]
    assert isinstance(new, ocn.ImmersedBoundaryGrid) and new.halo_size == (4, 0, 4) and new.size == ibg.size
    assert np.array_equal(new.immersed_cell_mask(), _cells(ocn, "G3")[1])
    assert new.immersed_boundary == IC.immersed_grid(ocn, None, "G3").immersed_boundary
    # a grid that already has the halo is taken as it is, with the solver's warning only
    ibg4 = IC.immersed_grid(ocn, None, "G1")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(_Stop) as stop:
            ocn.NonhydrostaticModel(grid=ibg4, tracers=())
    assert stop.value.args[0] is ibg4 and len(caught) == 1 and "FFT-based" in str(caught[0].message)


def test_refusals(ocn, monkeypatch):
    """everything an immersed grid does not serve raises NotImplementedError that names ImmersedBoundaryGrid and the feature, in Python,
    before any handle exists"""
    _no_handle(monkeypatch, ocn)
    ibg = IC.immersed_grid(ocn, None, "G1")
    F = ocn.FieldBoundaryConditions

    def refused(feature, make):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(NotImplementedError, match=feature) as e:
                make()
        assert "ImmersedBoundaryGrid" in str(e.value), feature

    model = lambda **kw: ocn.NonhydrostaticModel(grid=ibg, tracers=("b",), **kw)               # noqa: E731
    refused("PartialCellBottom", lambda: ocn.PartialCellBottom(-0.5, minimum_fractional_cell_height=0.2))
    refused("immersed", lambda: F(immersed=ocn.ValueBoundaryCondition(0.0)))
    refused("ImmersedBoundaryCondition", lambda: ocn.ImmersedBoundaryCondition(bottom=ocn.ValueBoundaryCondition(0.0)))
    refused("active_cells_map", lambda: ocn.ImmersedBoundaryGrid(IC.underlying_grid(ocn, None, "G1"), ocn.GridFittedBottom(-0.5), active_cells_map=True))
    refused("AnisotropicMinimumDissipation", lambda: model(closure=ocn.AnisotropicMinimumDissipation()))
    refused("Smagorinsky", lambda: model(closure=ocn.SmagorinskyLilly()))
    refused("DynamicSmagorinsky", lambda: model(closure=ocn.DynamicSmagorinsky(averaging=(1, 2))))
    refused("VerticallyImplicitTimeDiscretization", lambda: model(closure=ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=1e-3, κ=1e-3)))
    refused("background_fields", lambda: model(background_fields={"b": lambda x, y, z: z + 0 * x + 0 * y}))
    refused("stokes_drift", lambda: model(stokes_drift=ocn.UniformStokesDrift(dz_us=lambda z, t: 0.1)))
    refused("particles", lambda: model(particles=ocn.LagrangianParticles(x=[0.5], y=[0.5], z=[-0.1])))
    ibg2 = IC.immersed_grid(ocn, None, "G2")
    refused("scheme", lambda: ocn.NonhydrostaticModel(grid=ibg2, tracers=(), boundary_conditions={
        "u": F(east=ocn.OpenBoundaryCondition(0.1, scheme=ocn.PerturbationAdvection()))}))
    refused("gravity_unit_vector", lambda: model(buoyancy=ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=(0.0, np.sin(0.1), -np.cos(0.1)))))
    refused("ConstantCartesianCoriolis", lambda: model(coriolis=ocn.ConstantCartesianCoriolis(fx=0.0, fy=0.1, fz=1.0)))
    # diagnostics and time averages of operands on an immersed grid, and the checkpointer
    field = type("F", (ocn.Field,), {"__init__": lambda self: None, "__del__": lambda self: None})()
    field.grid, field.loc = ibg, (ocn.Center,) * 3
    refused("diagnostic", lambda: ocn.Average(field, dims=(1, 2)))
    refused("diagnostic", lambda: ocn.Integral(field))
    refused("diagnostic", lambda: field * 2.0)
    refused("diagnostic", lambda: ocn.dx(field))
    refused("diagnostic", lambda: ocn.WindowedTimeAverage(field, schedule=ocn.AveragedTimeInterval(1.0, window=0.5)))
    holder = type("M", (), {"grid": ibg})()
    refused("checkpointer", lambda: ocn.write_checkpoint(holder, "unused.npz"))
    refused("checkpointer", lambda: ocn.set_from_checkpoint(holder, "unused.npz"))
    # a grid that is no plain grid cannot be wrapped
    with pytest.raises(ValueError, match="non-immersed"):
        ocn.ImmersedBoundaryGrid(ibg, ocn.GridFittedBottom(-0.5))
    # what IS served constructs up to the handle
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(_Stop):
            ocn.NonhydrostaticModel(grid=ibg, tracers=("b", "c"), timestepper="QuasiAdamsBashforth2", buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=0.3),
                                    closure=ocn.ScalarDiffusivity(ν=1e-3, κ=2e-3), forcing={"c": np.zeros(ibg.size)},
                                    boundary_conditions={"b": F(top=ocn.FluxBoundaryCondition(0.1), bottom=ocn.ValueBoundaryCondition(0.0))})


def test_library_exports_the_new_symbols(ocn):
    lib = C.CDLL(ocn._lib.SO_PATH)
    for name in ("ocn_grid_set_immersed_boundary", "ocn_grid_get_immersed_flags", "ocn_mask_immersed_field"):
        assert hasattr(lib, name) and name in ocn._lib.SYMBOLS
