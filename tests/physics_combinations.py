"""Seeded mixed-physics models (test infrastructure; no device code): the draw of tests/test_physics_combinations_host.py and
tests/test_gpu_physics_combinations.py, the model and the composed yardstick of a drawn description, and the answers the plan's report
keys must give for it by the rules of include/ocn_mi355x.h.

draw(case) is a plain dict from np.random.default_rng(SEED + case), case = 0 .. N_CASES - 1:
  grid         "ppb" (Periodic, Periodic, Bounded) 8 x 6 x 10 tanh-stretched | "bbb" (Bounded)³ 7 x 6 x 8 stretched | "pfb" (Periodic, Flat,
               Bounded) 8 x 1 x 8 | "ppp" (Periodic)³ 8 x 6 x 6: no side longer than 10
  halo         (3, 3, 3) or one of the asymmetric halo_cases.HALOS (0 along a Flat direction)
  timestepper  "RungeKutta3" | "QuasiAdamsBashforth2"
  ntracers     1 (b) or 2 (b, S)
  closure      None | "scalar" (ScalarDiffusivity, ν ≠ κ_b ≠ κ_S) | "scalar_vi" (VerticallyImplicitTimeDiscretization: Bounded z only)
  coriolis     None | "fplane" | "cartesian"
  tilted       BuoyancyTracer on b, with or without a gravity_unit_vector of three nonzero components
  stokes       helpers.order_one_stokes_drift or none (no grid of the draw has a Flat z)
  background   a non-empty subset of (u, v, b), or ()
  forcing      the name of the one field with an array forcing, or None
  bcs          ((tracer, side, "flux", value), (tracer, side, "value", value)) on two different tracer walls, or () (always () without walls)
  particles    a handful of positions as fractions of the domain, or ()
Everything the library refuses (a Flat z with a drift, the implicit discretisation on a Periodic z, a condition on a side without a wall, a
halo deeper than the grid, partitioned grids) is left out of the draw, not caught: refusals(d) lists what a description would be refused
for and is empty for every drawn one. SEED is the smallest seed whose 12 draws meet every condition of the host test."""
import numpy as np

import halo_cases as HC
from helpers import order_one_stokes_drift, smooth_state

SEED = 86
N_CASES = 12
GRIDS = {"ppb": (HC.PPB, (8, 6, 10), True), "bbb": (HC.BBB, (7, 6, 8), True), "pfb": (HC.PFB, (8, 1, 8), False), "ppp": (HC.PPP, (8, 6, 6), False)}
HALOS = (HC.BASE,) + HC.HALOS[:3]
TIMESTEPPERS = ("RungeKutta3", "QuasiAdamsBashforth2")
NU, KAPPA = 2e-3, {"b": 5e-3, "S": 1e-3}
FCOR, CARTESIAN, GVEC = 0.7, (0.3, -1.1, 0.7), (0.48, -0.6, -0.64)
N2, THETA = 0.8, 0.3
SIDES = (("west", "east"), ("south", "north"), ("bottom", "top"))
N_PARTICLES = 6
RESTITUTION = 0.5
# the on / off features of the coverage conditions; `vertically_implicit` implies `closure`, `cartesian_coriolis` implies `coriolis`
FEATURES = ("asymmetric_halo", "ab2", "two_tracers", "closure", "vertically_implicit", "coriolis", "cartesian_coriolis", "tilted_gravity",
            "stokes_drift", "background", "forcing", "boundary_conditions", "particles")


def _walls(grid):
    return [s for d, pair in enumerate(SIDES) if GRIDS[grid][0][d] == "Bounded" for s in pair]


def draw(case):
    rng = np.random.default_rng(SEED + case)
    on = lambda p=0.55: bool(rng.random() < p)                                           # noqa: E731
    d = {"case": case, "grid": list(GRIDS)[rng.integers(len(GRIDS))]}
    topology, size, _ = GRIDS[d["grid"]]
    halo = HALOS[rng.integers(1, len(HALOS))] if on(0.5) else HC.BASE
    d["halo"] = tuple(0 if t == "Flat" else h for h, t in zip(halo, topology))
    d["timestepper"] = TIMESTEPPERS[int(on(0.5))]
    d["ntracers"] = 2 if on(0.5) else 1
    names = ("b", "S")[:d["ntracers"]]
    closures = ("scalar", "scalar_vi") if topology[2] == "Bounded" else ("scalar",)
    d["closure"] = closures[rng.integers(len(closures))] if on(0.65) else None
    d["coriolis"] = ("fplane", "cartesian")[rng.integers(2)] if on(0.65) else None
    d["tilted"] = on()
    d["stokes"] = on()
    subset = [n for n in ("u", "v", "b") if on(0.5)] or [("u", "v", "b")[rng.integers(3)]]
    d["background"] = tuple(subset) if on() else ()
    d["forcing"] = (("u", "v", "w") + names)[rng.integers(3 + len(names))] if on() else None
    walls = _walls(d["grid"])
    d["bcs"] = ()
    if walls and on(0.6):
        spots = [(n, s) for n in names for s in walls]
        a, b = rng.choice(len(spots), size=2, replace=False)
        d["bcs"] = (spots[a] + ("flux", 0.03), spots[b] + ("value", 0.4))
    d["particles"] = tuple(tuple(float(x) for x in p) for p in rng.uniform(0.1, 0.9, (N_PARTICLES, 3))) if on() else ()
    return d


def features(d):
    return {"asymmetric_halo": any(h not in (0, 3) for h in d["halo"]), "ab2": d["timestepper"] == "QuasiAdamsBashforth2",
            "two_tracers": d["ntracers"] == 2, "closure": d["closure"] is not None, "vertically_implicit": d["closure"] == "scalar_vi",
            "coriolis": d["coriolis"] is not None, "cartesian_coriolis": d["coriolis"] == "cartesian", "tilted_gravity": d["tilted"],
            "stokes_drift": d["stokes"], "background": bool(d["background"]), "forcing": d["forcing"] is not None,
            "boundary_conditions": bool(d["bcs"]), "particles": bool(d["particles"])}


def refusals(d):
    """why the library (or the reference) would refuse the description; empty for everything draw() returns"""
    topology, size, _ = GRIDS[d["grid"]]
    out = []
    if d["stokes"] and topology[2] == "Flat":
        out.append("a UniformStokesDrift on a Flat z")
    if d["closure"] == "scalar_vi" and topology[2] != "Bounded":
        out.append("VerticallyImplicitTimeDiscretization on a z that is not Bounded")
    if any(h > n for h, n in zip(d["halo"], size)) or any((h == 0) != (t == "Flat") for h, t in zip(d["halo"], topology)):
        out.append("a halo deeper than the grid, or a halo along a Flat direction")
    if any(side not in _walls(d["grid"]) for _, side, _, _ in d["bcs"]):
        out.append("a Flux or Value condition on a side without a wall")
    if len({(n, s) for n, s, _, _ in d["bcs"]}) != len(d["bcs"]):
        out.append("two conditions on one side")
    names = ("u", "v", "w", "b", "S")[:3 + d["ntracers"]]
    if any(n not in names for n in d["background"] + ((d["forcing"],) if d["forcing"] else ()) + tuple(n for n, _, _, _ in d["bcs"])):
        out.append("a field the model does not have")
    return out


def expected_plan(d, fused=True):
    """the report keys of ocn_model_get_option by the rules of include/ocn_mi355x.h. Every drawn model has a buoyancy, so a physics epilogue
    exists on the default path: a forcing takes the stand-alone pass (3) and keeps the substep out of the tendency launches, the substep
    otherwise rides in the epilogue, the Stokes terms are inside it (2). fused = False: fused_epilogue = 0 and fuse_substep = 0."""
    topology = GRIDS[d["grid"]][0]
    role_kernel = topology[0] == "Periodic" and topology[1] == "Periodic" and "Flat" not in topology
    march = (fused and d["closure"] == "scalar" and d["coriolis"] != "cartesian" and not d["tilted"] and not d["stokes"] and
             "Flat" not in topology)
    return {"forcing_path": 3 if d["forcing"] else 0,
            "background_tendency_path": 0 if not d["background"] else (2 if role_kernel else 1),
            "stokes_path": 0 if not d["stokes"] else (2 if fused else 1),
            "fuse_substep_active": int(fused and not d["forcing"]),
            "epilogue_march_active": int(march),
            "coriolis_kind": {None: 0, "fplane": 1, "cartesian": 2}[d["coriolis"]],
            "tilted_gravity": int(d["tilted"]),
            "vertically_implicit": int(d["closure"] == "scalar_vi")}


# ---------------------------------------------------------------------------------------------------------------------
# the pieces of a description that the model and the yardstick share (host arithmetic only)
# ---------------------------------------------------------------------------------------------------------------------
BACKGROUNDS = {"u": lambda x, y, z: 0.3 * np.tanh(4 * (z + 0.5)) + 0 * x + 0 * y,
               "v": lambda x, y, z: 0.2 * np.tanh(4 * (z + 0.5)) + 0 * x + 0 * y,
               "b": lambda x, y, z: N2 * (x * np.sin(THETA) + z * np.cos(THETA)) + 0 * y}


def make_grid(ocn, arch, d):
    """arch = None: host metadata only"""
    topology, size, stretched = GRIDS[d["grid"]]
    return HC.make_grid(ocn, arch, topology, size, d["halo"], stretched)


def make_oracle_grid(O, d):
    topology, size, stretched = GRIDS[d["grid"]]
    return HC.make_oracle_grid(O, topology, size, d["halo"], stretched)


def tracer_names(d):
    return ("b", "S")[:d["ntracers"]]


def yard_name(d, name):
    return name if name in "uvw" else "c%d" % tracer_names(d).index(name)


def locations(ocn, d):
    F, Cn = ocn.Face, ocn.Center
    loc = {"u": (F, Cn, Cn), "v": (Cn, F, Cn), "w": (Cn, Cn, F)}
    loc.update({n: (Cn, Cn, Cn) for n in tracer_names(d)})
    return loc


def forcing_array(ocn, grid, d):
    if d["forcing"] is None:
        return None
    return 0.3 * np.random.default_rng(SEED + 1000 + d["case"]).standard_normal(tuple(grid.size))      # Forcing(array): size(grid), whatever the location


def particle_positions(geometry, d):
    """the drawn fractions on the domain of the grid; along a Flat direction the one coordinate there is"""
    import particles_reference as P
    frac = np.array(d["particles"])
    return [np.full(len(frac), geometry.xL[k]) if geometry.topo[k] == P.FLAT else geometry.xL[k] + frac[:, k] * geometry.length(k) for k in range(3)]


def initial_values(grid, d, ocn):
    loc = locations(ocn, d)
    vals = smooth_state({("T" if n == "b" else n): grid.nodes(l) for n, l in loc.items()}, 17)
    vals["b"] = vals.pop("T")
    return vals


def build_model(ocn, arch, d, options=None):
    """-> grid, model (state set and projected)"""
    import particles_reference as P
    grid = make_grid(ocn, arch, d)
    names = tracer_names(d)
    closure = None
    if d["closure"]:
        kappa = {n: KAPPA[n] for n in names}
        closure = (ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=NU, κ=kappa) if d["closure"] == "scalar_vi"
                   else ocn.ScalarDiffusivity(ν=NU, κ=kappa))
    coriolis = {None: None, "fplane": ocn.FPlane(f=FCOR),
                "cartesian": ocn.ConstantCartesianCoriolis(fx=CARTESIAN[0], fy=CARTESIAN[1], fz=CARTESIAN[2])}[d["coriolis"]]
    buoyancy = ocn.BuoyancyForce(ocn.BuoyancyTracer(), gravity_unit_vector=GVEC) if d["tilted"] else ocn.BuoyancyTracer()
    bcs = {}
    for name, side, kind, value in d["bcs"]:
        bc = ocn.FluxBoundaryCondition(value) if kind == "flux" else ocn.ValueBoundaryCondition(value)
        bcs.setdefault(name, {})[side] = bc
    forcing = forcing_array(ocn, grid, d)
    particles = None
    if d["particles"]:
        x, y, z = particle_positions(P.Geometry.of_grid(grid), d)
        particles = ocn.LagrangianParticles(x=x, y=y, z=z, restitution=RESTITUTION)
    model = ocn.NonhydrostaticModel(grid=grid, tracers=names, timestepper=d["timestepper"], buoyancy=buoyancy, coriolis=coriolis, closure=closure,
                                    boundary_conditions={n: ocn.FieldBoundaryConditions(**s) for n, s in bcs.items()} or None,
                                    forcing={d["forcing"]: forcing} if d["forcing"] else None,
                                    background_fields={n: BACKGROUNDS[n] for n in d["background"]} or None,
                                    stokes_drift=order_one_stokes_drift(ocn) if d["stokes"] else None, particles=particles)
    for k, v in (options or {}).items():
        model.set_option(k, v)
    ocn.set_model(model, **initial_values(grid, d, ocn))
    return grid, model


def build_yardstick(ocn, O, d, grid):
    """ParticlesOrchestrated (StokesOrchestrated without particles) of the description; `grid`: the package's grid of make_grid (host
    metadata is enough). The background arrays are the package's own host evaluation of the functions, the tables its drift's."""
    import particles_reference as P
    import stokes_reference as S
    from oldoceananigans_jl_amd.background_fields import regularize_background_field
    names = tracer_names(d)
    loc = locations(ocn, d)
    g_cpu = make_oracle_grid(O, d)
    forcing = forcing_array(ocn, grid, d)
    bcs = {}
    for name, side, kind, value in d["bcs"]:
        bcs.setdefault(yard_name(d, name), {})[side] = (kind, value)
    kw = dict(stokes_tables=order_one_stokes_drift(ocn).tables(grid) if d["stokes"] else None,
              background={yard_name(d, n): regularize_background_field(loc[n], BACKGROUNDS[n], grid) for n in d["background"]} or None,
              buoyancy_index=0, fcor=FCOR if d["coriolis"] == "fplane" else None, cartesian=CARTESIAN if d["coriolis"] == "cartesian" else None,
              gravity_unit_vector=GVEC if d["tilted"] else None, forcing={yard_name(d, d["forcing"]): forcing} if d["forcing"] else None,
              closure="vi" if d["closure"] == "scalar_vi" else "numpy", bcs=bcs or None)
    nu = NU if d["closure"] else 0.0
    kappa = tuple(KAPPA[n] if d["closure"] else 0.0 for n in names)
    if d["particles"]:
        geometry = P.Geometry.of_grid(grid)
        x, y, z = particle_positions(geometry, d)
        yard = P.ParticlesOrchestrated(O, g_cpu, len(names), nu, kappa, geometry=geometry, particles=dict(x=x, y=y, z=z), restitution=RESTITUTION, **kw)
    else:
        yard = S.StokesOrchestrated(O, g_cpu, len(names), nu, kappa, **kw)
    vals = initial_values(grid, d, ocn)
    yard.set(**{yard_name(d, n): v for n, v in vals.items()})
    return yard


def step(yard, d, dt):
    yard.time_step(dt) if d["timestepper"] == "RungeKutta3" else yard.time_step_ab2(dt)
