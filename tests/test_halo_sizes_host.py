"""CPU: what tests/test_gpu_halo_sizes.py rests on when it runs the device at halos other than (3, 3, 3) (tests/halo_cases.py).

  * the oracle's interiors do not depend on the halo depth: 3 RK3 and 3 AB2 steps and the stage tendencies at every HALOS entry equal
    those at (3, 3, 3) with `==` -- so the oracle at halo H is a valid reference for the device at halo H;
  * the numpy restatements of the feature kernels return the same interiors at every halo;
  * the host plumbing (with_halo, total_size, interior_size, nodes, the node tables handed to the library) is halo-general.

No GPU, no tolerance: everything here is `==`."""
import numpy as np
import pytest

import halo_cases as HC
from helpers import smooth_state

CNAMES = ["u", "v", "w", "c0", "c1"]
ORO_LOCS = {"u": (1, 0, 0), "v": (0, 1, 0), "w": (0, 0, 1), "c0": (0, 0, 0), "c1": (0, 0, 0), "p": (0, 0, 0)}
_cache = {}


@pytest.fixture(scope="module")
def ocn_host():
    import oldoceananigans_jl_amd as ocn
    return ocn


def _locs(ocn):
    F, Cn = ocn.Face, ocn.Center
    return {"u": (F, Cn, Cn), "v": (Cn, F, Cn), "w": (Cn, Cn, F), "T": (Cn,) * 3, "S": (Cn,) * 3}


def _oracle_model(oracle, g, physics):
    m = oracle.Model(g, 2)
    if physics == "amd":
        m.set_amd()
        m.set_coriolis(0.3)
        m.set_seawater_buoyancy(alpha=2e-4, beta=8e-4)
    elif physics == "scalar":
        m.set_closure(nu=2e-3, kappa=[1e-3, 5e-4])
        m.set_coriolis(0.3)
        m.set_seawater_buoyancy(alpha=2e-4, beta=8e-4)
    return m


def _oracle_run(ocn, oracle, case, halo, stepper):
    """-> interiors of u, v, w, c0, c1, p after 3 steps, and of the stage tendencies G* of one more update_state"""
    key = (case, halo, stepper)
    if key in _cache:
        return _cache[key]
    topology, size, stretched, physics = HC.ORACLE_CASES[case]
    grid = HC.make_grid(ocn, None, topology, size, halo, stretched)
    g = HC.make_oracle_grid(oracle, topology, size, halo, stretched)
    assert g.H == tuple(halo)
    m = _oracle_model(oracle, g, physics)
    vals = smooth_state({n: grid.nodes(loc) for n, loc in _locs(ocn).items()}, 1234)
    m.set(**{cn: vals[n] for cn, n in zip(CNAMES, _locs(ocn))})
    dt = 0.1 * min(grid.Δxᶜᵃᵃ, grid.Δyᵃᶜᵃ, float(np.min(grid.Δzᵃᵃᶜ))) / 0.6
    for n in range(3):
        if stepper == "rk3":
            m.time_step(dt)
        else:
            m.time_step_ab2(dt if n < 2 else 0.7 * dt)
    out = {n: HC.interior(g, m.field(n), ORO_LOCS[n]).copy() for n in CNAMES + ["p"]}
    m.update_state(True)
    out |= {"G" + n: HC.interior(g, m.field("G" + n), ORO_LOCS[n]).copy() for n in CNAMES}
    _cache[key] = out
    return out


@pytest.mark.parametrize("stepper", ["rk3", "ab2"])
@pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("case", list(HC.ORACLE_CASES))
def test_oracle_interiors_do_not_depend_on_the_halo(ocn_host, oracle, case, halo, stepper):
    ref = _oracle_run(ocn_host, oracle, case, HC.BASE, stepper)
    got = _oracle_run(ocn_host, oracle, case, halo, stepper)
    assert set(got) == set(ref)
    for n in ref:
        assert np.abs(ref[n]).max() > 0 or n == "Gw" or n == "p", (case, n)
        assert got[n].shape == ref[n].shape, (case, halo, n)
        assert np.array_equal(got[n], ref[n]), (case, halo, stepper, n, int((got[n] != ref[n]).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# host plumbing
# ---------------------------------------------------------------------------------------------------------------------
PLUMBING = [("ppp", HC.PPP, (12, 10, 8), False), ("ppb", HC.PPB, (12, 10, 8), True), ("bbb", HC.BBB, (9, 8, 7), False),
            ("bpb", HC.BPB, (12, 10, 8), True), ("pfb", HC.PFB, (16, 1, 8), True)]


@pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("name,topology,size,stretched", PLUMBING, ids=[p[0] for p in PLUMBING])
def test_grid_shapes_and_nodes_at_other_halos(ocn_host, name, topology, size, stretched, halo):
    ocn = ocn_host
    base = HC.make_grid(ocn, None, topology, size, HC.BASE, stretched)
    grid = ocn.grids.with_halo(halo, base)
    flat = [t == "Flat" for t in topology]
    H = tuple(0 if f else h for h, f in zip(halo, flat))
    assert grid.halo_size == H and grid.size == base.size and grid.topology == base.topology
    direct = HC.make_grid(ocn, None, topology, size, halo, stretched)
    for loc in list(_locs(ocn).values()) + [(ocn.Face, ocn.Face, ocn.Face)]:
        inner, total = grid.interior_size(loc), grid.total_size(loc)
        assert inner == base.interior_size(loc)
        assert total == tuple(n + 2 * h for n, h in zip(inner, H))
        assert total == direct.total_size(loc)
        a = np.arange(np.prod(total), dtype=np.float64).reshape(total, order="F")
        core = HC.interior(grid, a, loc)
        assert core.shape == inner
        assert core[0, 0, 0] == H[0] + total[0] * (H[1] + total[1] * H[2])        # the first interior point sits at (Hx, Hy, Hz)
        # interior nodes: the same points of space whatever the halo, bit for bit
        for got, want in zip(grid.nodes(loc), base.nodes(loc)):
            assert got.shape == want.shape and np.array_equal(got, want), (name, halo, loc)
    # reduced locations have one point and no halo
    assert grid.total_size((None, None, ocn.Center)) == (1, 1, size[2] + 2 * H[2])
    # the spacing tables start at k = 1 - Hz: the interior entries are those of the (3, 3, 3) grid
    for got, want in ((grid.Δzᵃᵃᶜ, base.Δzᵃᵃᶜ), (grid.Δzᵃᵃᶠ, base.Δzᵃᵃᶠ)):
        assert got.shape == (size[2] + 2 * H[2] + 1,)
        assert np.array_equal(got[H[2]:H[2] + size[2]], want[base.Hz:base.Hz + size[2]])
    with pytest.raises(ValueError):
        ocn.grids.with_halo(tuple(n + 1 for n in size), base)


@pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
def test_halo_larger_than_a_direction_is_refused_in_each_direction(ocn_host, halo):
    for d in range(3):
        size = [max(halo)] * 3
        size[d] = halo[d] - 1
        with pytest.raises(ValueError):
            HC.make_grid(ocn_host, None, HC.PPP, tuple(size), halo)
        size[d] = halo[d]
        HC.make_grid(ocn_host, None, HC.PPP, tuple(size), halo)              # N == H is accepted


class _RecordingLib:
    """stands in for the library while a grid handle is created: records what ocn_grid_create, ocn_grid_set_nodes and
    ocn_grid_set_node_tables are handed (sizes, halos, the node coordinates and the node tables as numpy copies)"""

    def __init__(self, N):
        self.N, self.calls = N, {}

    def ocn_grid_create(self, handle, N, H, topo, L, dx, dy, dz, zc, zf):
        self.calls["create"] = (tuple(N), tuple(H), tuple(topo), tuple(L), dx, dy, dz)
        return 0

    def ocn_grid_set_nodes(self, handle, f0, c0, f1, zf, zc):
        self.calls["nodes"] = (tuple(f0), tuple(c0), tuple(f1))
        return 0

    def ocn_grid_set_node_tables(self, handle, faces, centers):
        self.calls["tables"] = None          # the arrays are kept on the grid (grid._node_tables); read there
        return 0

    def ocn_grid_destroy(self, handle):
        return 0


@pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("name,topology,size,stretched", PLUMBING, ids=[p[0] for p in PLUMBING])
def test_node_tables_handed_to_the_library(ocn_host, monkeypatch, name, topology, size, stretched, halo):
    """the node tables and corner nodes that ocn_grid_set_node_tables / ocn_grid_set_nodes receive are cut out of the haloed coordinate
    arrays at [H : H + N (+ 1)]: at every halo they are the values the (3, 3, 3) grid hands over for the same interior points"""
    ocn = ocn_host
    got = {}
    for h in (HC.BASE, halo):
        grid = HC.make_grid(ocn, None, topology, size, h, stretched)
        rec = _RecordingLib(size)
        monkeypatch.setattr(ocn._lib, "lib", lambda rec=rec: rec)
        monkeypatch.setattr(ocn._lib, "check", lambda rc: None)
        assert grid.handle is not None
        assert rec.calls["create"][0] == tuple(size) and rec.calls["create"][1] == grid.halo_size
        got[h] = (rec.calls["nodes"], grid._node_tables, rec.calls["create"][3:])
        grid._handle = None                  # nothing to destroy
    (nodes0, tables0, metric0), (nodes1, tables1, metric1) = got[HC.BASE], got[halo]
    assert nodes0 == nodes1 and metric0 == metric1
    for d in range(3):
        n = 1 if topology[d] == "Flat" else size[d]
        assert tables1[0][d].shape == ((1,) if topology[d] == "Flat" else (n + 1,)) and tables1[1][d].shape == (n,)
        assert np.array_equal(tables1[0][d], tables0[0][d]) and np.array_equal(tables1[1][d], tables0[1][d]), (name, halo, d)


# ---------------------------------------------------------------------------------------------------------------------
# the numpy restatements of the feature kernels
# ---------------------------------------------------------------------------------------------------------------------
# One state per grid: seeded random INTERIOR values (the same at every halo), the halos filled by the oracle's default fill at that halo. Each
# restatement is evaluated on host-only grids (arch = None); what it returns on the interior must not depend on the halo depth.
REST_GRIDS = {"ppb": (HC.PPB, (12, 10, 8), True), "bbb": (HC.BBB, (9, 8, 7), False)}
REST_LOCS = {"u": (1, 0, 0), "v": (0, 1, 0), "w": (0, 0, 1), "c": (0, 0, 0), "S": (0, 0, 0), "Gu": (1, 0, 0), "Gv": (0, 1, 0), "Gw": (0, 0, 1), "Gc": (0, 0, 0)}


def _rest_state(ocn, oracle, gid, halo):
    key = ("rest", gid, halo)
    if key not in _cache:
        topology, size, stretched = REST_GRIDS[gid]
        grid = HC.make_grid(ocn, None, topology, size, halo, stretched)
        g = HC.make_oracle_grid(oracle, topology, size, halo, stretched)
        rng = np.random.default_rng(99)
        P = {}
        for n, loc in REST_LOCS.items():
            a = g.zeros(loc)
            core = g.interior(a, loc)
            core[...] = rng.uniform(-1.0, 1.0, core.shape) + (35.0 if n == "S" else 0.0)
            g.fill_halo_regions(a, loc)
            P[n] = a
        _cache[key] = (grid, g, P)
    return _cache[key]


def _cls(ocn, code):
    return tuple(ocn.Face if c else ocn.Center for c in code)


def _restatement_results(ocn, oracle, gid, halo, which):
    """-> dict label -> interior array (or position / face arrays that must not depend on the halo)"""
    grid, g, P = _rest_state(ocn, oracle, gid, halo)
    core = lambda a, n: HC.interior(g, a, REST_LOCS[n]).copy()          # noqa: E731
    out = {}
    if which == "diagnostics":
        import diagnostics_reference as D
        F, Cn = ocn.Face, ocn.Center
        wu = D.Operand(3, P["w"], P["u"], None, None, _cls(ocn, REST_LOCS["w"]), _cls(ocn, REST_LOCS["u"]), (F, Cn, F))
        plain = D.Operand(0, P["u"], None, None, None, _cls(ocn, REST_LOCS["u"]), None, _cls(ocn, REST_LOCS["u"]))
        scaled = D.Operand(4, None, P["c"], 2.0, None, None, (Cn, Cn, Cn), (Cn, Cn, Cn))
        for label, op in (("w*u", wu), ("u", plain), ("2/c", scaled)):
            out[label] = D.compute_operation(grid, op)
            for mask in (1, 2, 4, 3, 5, 6, 7):
                out[label, "max", mask] = D.reduce_operation(grid, op, "maximum", mask, False, True)
                out[label, "sum", mask] = D.reduce_operation(grid, op, "sum", mask, True)
                out[label, "avg", mask] = D.reduce_operation(grid, op, "average", mask, True)
            for dim in range(3):
                out[label, "cumulative", dim] = D.accumulate_operation(grid, op, dim, dim == 1, True)
    elif which == "forcing_function":
        import forcing_function_reference as R
        deps = [(P[n], _cls(ocn, REST_LOCS[n])) for n in ("u", "v", "w", "c")]
        f = lambda x, y, z, t, u, v, w, T: x * z + t * u - v / (1.5 + w * T) + ocn.ifelse(w > u, ocn.min_(u, y), ocn.max_(v, T))          # noqa: E731
        for n in ("u", "v", "w", "c"):
            out[n] = R.evaluate(f, grid, _cls(ocn, REST_LOCS[n]), deps, 1.75)
    elif which == "boundary_function":
        import boundary_function_reference as R
        deps = [(P[n], _cls(ocn, REST_LOCS[n])) for n in ("u", "v", "w", "c")]
        walls = [s for s in range(6) if grid.topology[s // 2] is ocn.Bounded]
        f = lambda a, b, t, u, v, w, T: -2e-3 * ocn.sqrt(u ** 2 + (v + 0.1) ** 2) * u + a * t - b / 3.0 + abs(w) * (T >= 0.25)              # noqa: E731
        for side in walls:
            for n in ("u", "v", "w", "c"):
                out[side, n] = R.evaluate(f, grid, _cls(ocn, REST_LOCS[n]), side, deps, 1.75)
    elif which == "particles":
        import particles_reference as R
        geo = R.Geometry.of_grid(grid)
        rng = np.random.default_rng(5)
        pos = []
        for d in range(3):
            lo, hi = geo.xL[d], geo.xR[d]
            dl = geo.d[d] if not (d == 2 and geo.zf is not None) else geo.zf[1] - geo.zf[0]
            a = rng.uniform(lo, hi, 64)
            a[:6] = [lo, hi, lo + 0.2 * dl, lo + 0.45 * dl, hi - 0.3 * dl, hi - 0.05 * dl]         # the first and last half cells read the halo
            pos.append(rng.permutation(a))
        for n, loc in (("c", R.LOC_C), ("u", R.LOC_U), ("v", R.LOC_V), ("w", R.LOC_W)):
            out["interpolate", n] = R.interpolate(geo, P[n], loc, *pos)
        for Cr in (1.0, 0.5):
            out["advect", Cr] = np.array(R.advect(geo, *pos, P["u"], P["v"], P["w"], 2.5, Cr, None))
        assert (geo.N, geo.H) == (grid.size, grid.halo_size)
    elif which == "vertically_implicit":
        import vertically_implicit_reference as R
        m = R.Metrics.of_grid(grid)
        dt = 100.0 * float(m.dzc[m.H[2]:m.H[2] + m.N[2]].min()) ** 2 / 1.7
        for n in "uvwc":
            out["solve", n] = core(R.implicit_step(m, P[n].copy(order="F"), R.LOCS[n], 1.7, dt), n)
            for vi in (True, False):
                out["explicit", n, vi] = core(R.explicit_part(m, n, P, P["c"], 0.37, P["G" + n].copy(order="F"), vi=vi), n)
    elif which == "smagorinsky":
        import smagorinsky_reference as R
        m = R.Metrics(grid)
        out["constant"] = R.viscosity(m, P["u"], P["v"], P["w"], 0.16)
        out["lilly"] = R.viscosity(m, P["u"], P["v"], P["w"], 0.16, Cb=0.5, buoyancy=("seawater", P["c"], P["S"], R.GRAV, R.ALPHA, R.BETA))
        assert out["constant"].shape == grid.size and out["constant"].max() > 0
    elif which == "stokes":
        import stokes_reference as R
        import vertically_implicit_reference as V
        m = V.Metrics.of_grid(grid)
        drift = ocn.UniformStokesDrift(dz_us=lambda z, t: 0.7 * (1.0 + z), dz_vs=lambda z, t: -0.4 * z * z, dt_us=lambda z, t: 0.05 * z, dt_vs=lambda z, t: 0.02 * (1 + z))
        G = R.add_stokes_drift(m, drift.tables(grid), P, {n: P["G" + n].copy(order="F") for n in "uvw"})
        out = {n: core(G[n], n) for n in "uvw"}
    elif which == "background":
        import background_reference as R
        import vertically_implicit_reference as V
        m = V.Metrics.of_grid(grid)
        adv = (P["Gu"], P["Gv"], P["Gw"])           # advecting != advected
        for n in "uvwc":
            for accumulate in (False, True):
                out[n, accumulate] = core(R.advective_tendency(m, n, adv, P[n], G=P["G" + n].copy(order="F"), accumulate=accumulate), n)
    elif which == "open_boundary":
        import open_boundary_reference as R
        import vertically_implicit_reference as V
        m = V.Metrics.of_grid(grid)
        sides = [s for s in R.SIDES if m.topo[R.SIDES.index(s) // 2] == 1]
        for side in sides:
            n = R.NORMAL[side]
            for tin, tout, dt in ((0.3, 2.0, 0.02), (0.5, 0.0, 0.3), (0.3, 2.0, float("inf"))):
                out[side, tin, tout, dt] = core(R.step_side(m, P[n].copy(order="F"), side, 1.3, tin, tout, dt), n)
        conditions = {s: 0.4 for s in sides}
        out["inflow"] = np.array(R.mass_inflow(m, P, conditions, {}))
        U = {n: P[n].copy(order="F") for n in "uvw"}
        R.enforce(m, U, conditions, {s: (0.1, float("inf")) for s in sides})
        out |= {("enforce", n): core(U[n], n) for n in "uvw"}
    assert out
    return out


RESTATEMENTS = ["diagnostics", "forcing_function", "boundary_function", "particles", "vertically_implicit", "smagorinsky", "stokes", "background", "open_boundary"]


@pytest.mark.parametrize("halo", HC.HALOS, ids=HC.halo_id)
@pytest.mark.parametrize("gid", list(REST_GRIDS))
@pytest.mark.parametrize("which", RESTATEMENTS)
def test_restatements_do_not_depend_on_the_halo(ocn_host, oracle, which, gid, halo):
    if ("rest-result", which, gid) not in _cache:
        _cache["rest-result", which, gid] = _restatement_results(ocn_host, oracle, gid, HC.BASE, which)
    ref = _cache["rest-result", which, gid]
    got = _restatement_results(ocn_host, oracle, gid, halo, which)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape, (which, gid, halo, k)
        assert np.array_equal(got[k], ref[k]), (which, gid, halo, k, float(np.abs(got[k] - ref[k]).max()))
