"""Which tendency epilogue a model runs, for every combination of physics the setters can reach: the selection is checked, not the kernels'
interiors (those are pinned by test_gpu_parity.py, test_gpu_tilted.py, test_gpu_smagorinsky.py, test_gpu_stokes.py, ...).

One model per (ntracers, closure) on the (Periodic, Periodic, Bounded) 8 x 6 x 10 tanh-stretched grid of test_gpu_tilted.py with
helpers.smooth_state. Within the model the setters walk coriolis in {nothing, FPlane(0.7), ConstantCartesianCoriolis(0.3, -1.1, 0.7)} x
buoyancy in {nothing, BuoyancyTracer, linear SeawaterBuoyancy} x gravity_unit_vector in {none, (0.48, -0.6, -0.64)}, every replacement of
one Coriolis by another at least once. At every combination update_state!(compute_tendencies = true) runs three times -- the default path
(the fused epilogue, z-marching where it serves), epilogue_march = 0 (the per-value epilogue) and fused_epilogue = 0 (the stand-alone
kernels, which the epilogue's dispatch does not touch) -- and
  * Gu, Gv, Gw, Gc* of the three are np.array_equal and finite;
  * "epilogue_march_active", "coriolis_kind", "tilted_gravity" and "vertically_implicit" answer the rule of include/ocn_mi355x.h: marching
    iff there is a closure, it is not vertically implicit, ntracers <= 2, no ConstantCartesianCoriolis and no tilted buoyancy;
  * G differs from the G of the same state without physics whenever a term is on (an epilogue that did nothing fails).

The STOKES axis. At the same combination ocn_model_set_stokes_drift switches helpers.order_one_stokes_drift on ("stokes_drift" 1,
"stokes_path" 2, "epilogue_march_active" 0 whatever the closure): the default path is then the STOKES instantiation of the per-value
epilogue, and
  * Gu, Gv, Gw are np.array_equal over the whole parent array to stokes_reference.add_stokes_drift applied to the drift-free tendencies of
    the comparison above -- (G + curl) + ∂t on a tendency that holds everything up to the closure term, the order of
    nonhydrostatic_tendency_kernel_functions.jl:99-102 -- and every tracer tendency keeps the bits of its drift-free one;
  * fused_epilogue = 0 ("stokes_path" 1: the stand-alone physics kernels, then stokes_drift_kernel) gives the same bits;
  * Gu, Gv, Gw differ from the drift-free ones (an epilogue that skipped the Stokes terms fails);
  * ocn_model_set_stokes_drift(model, 0, NULLs) brings back the old answer of "epilogue_march_active" and the drift-free bits.

The substep that rides along (a.Gm, a.Un are run-time arguments: an update_state! alone never reaches that code). At the second and the
last entry of every Coriolis walk -- each (gravity, buoyancy) pair once with a Coriolis and once without -- one RK3 step is taken from the
saved state (fields and pressure restored, update_state!) by the model on its default path ("fuse_substep_active" 1) and by a twin that
got the same setters and has fused_epilogue = 0 ("fuse_substep_active" 0): fields, Gⁿ, G⁻ and pNHS are np.array_equal and finite. With the drift on at every such entry, with the drift off
where the plan marches; scalar_vi included (its implicit solve follows the substep on both paths).

No combination is exempt: every one is bit-identical across the paths, with and without the drift. The walk launches all 60 STOKES
instantiations, 59 of the 60 without the terms (the all-off one runs only for a model that has Flux conditions and nothing else:
test_gpu_boundary_function.py) and the 28 marching ones a model can reach -- the other 8 are BUOY or CLO 3 without a tracer (DESIGN.md 13
derives the counts from epilogue_slot and epilogue_march_slot)."""
import ctypes as C

import numpy as np
import pytest

from helpers import order_one_stokes_drift, smooth_state, tanh_faces
import stokes_reference as S
import vertically_implicit_reference as R

pytestmark = pytest.mark.gpu

OCN_ESTATE = -3                                            # include/ocn_mi355x.h
NAMES = ("T", "S", "c")
NU, KAPPA = 2e-3, (5e-3, 3e-3, 1e-3)
GRAV, ALPHA, BETA = 9.80665, 1.67e-4, 7.8e-4
GVEC = (0.48, -0.6, -0.64)
FPLANE, CARTESIAN = 0.7, (0.3, -1.1, 0.7)
CLOSURES = ("none", "scalar", "scalar_vi", "amd", "smagorinsky", "smagorinsky_lilly_pr")
# the Coriolis walks of consecutive (gravity, buoyancy) combinations, each starting from `nothing`: together they make every replacement
# (nothing -> FPlane -> Cartesian -> FPlane -> nothing, nothing -> Cartesian -> FPlane -> Cartesian -> nothing)
WALKS = ((1, 2, 1, 0), (2, 1, 2, 0))


def _doubles(values):
    return (C.c_double * len(values))(*values) if len(values) else None


def _model(ocn, arch, ntr):
    """the model without physics, its state set, and G of that state"""
    grid = ocn.RectilinearGrid(arch, size=(8, 6, 10), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded), x=(0.0, 1.0), y=(0.0, 1.0),
                               z=tanh_faces(10), halo=(3, 3, 3))
    model = ocn.NonhydrostaticModel(grid=grid, tracers=NAMES[:ntr])
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 17))
    return grid, model


def _tendencies(ocn, model):
    ocn.update_state(model, True)
    return [model.tendency(n).parent().copy() for n in model.fields()]


def _set_closure(L, model, closure, ntr):
    h = model.handle
    if closure in ("scalar", "scalar_vi"):
        # VerticallyImplicitTimeDiscretization may be named before the coefficients (ntr odd) or after them
        if closure == "scalar_vi" and ntr % 2:
            assert L.ocn_model_set_vertically_implicit(h, 1) == 0 and model.get_option("vertically_implicit") == 1
        assert L.ocn_model_set_closure(h, NU, _doubles(KAPPA[:ntr])) == 0
        if closure == "scalar_vi" and not ntr % 2:
            assert L.ocn_model_set_vertically_implicit(h, 1) == 0
    elif closure == "amd":
        assert L.ocn_model_set_amd(h, 1.0 / 12.0, _doubles((1.0 / 12.0, 0.1, 0.05)[:ntr])) == 0
    elif closure == "smagorinsky":
        assert L.ocn_model_set_smagorinsky(h, 0.16, 0.0, 0, _doubles((1.0,) * ntr)) == 0
    elif closure == "smagorinsky_lilly_pr":
        assert L.ocn_model_set_smagorinsky(h, 0.16, 1.0, 1, _doubles((0.7, 1.3, 1.0)[:ntr])) == 0


def _set_buoyancy(L, model, kind):
    if kind == 2:
        assert L.ocn_model_set_buoyancy(model.handle, 2, 0, 1, GRAV, ALPHA, BETA) == 0
    else:
        assert L.ocn_model_set_buoyancy(model.handle, kind, 0, 0, 0.0, 0.0, 0.0) == 0


def _set_coriolis(L, model, kind, previous):
    """coriolis = nothing through the setter of the kind that is being removed, so both `enabled = 0` arms are visited"""
    h = model.handle
    if kind == 1:
        assert L.ocn_model_set_coriolis(h, 1, FPLANE) == 0
    elif kind == 2:
        assert L.ocn_model_set_cartesian_coriolis(h, 1, *CARTESIAN) == 0
    elif previous == 2:
        assert L.ocn_model_set_cartesian_coriolis(h, 0, 0.0, 0.0, 0.0) == 0
    else:
        assert L.ocn_model_set_coriolis(h, 0, 0.0) == 0


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _set_drift(L, model, tables):
    dp = C.POINTER(C.c_double)
    args = [t.ctypes.data_as(dp) for t in tables] if tables is not None else [None] * 6
    assert L.ocn_model_set_stokes_drift(model.handle, int(tables is not None), *args) == 0


def _state_names(model):
    return ["u", "v", "w"] + ["c%d" % t for t in range(len(model.tracer_names))]


def _save(model):
    """the prognostic fields and the pressure: whole parent arrays"""
    return {n: model._field(n).parent() for n in _state_names(model) + ["p"]}


def _step_from(ocn, model, saved, dt):
    """one RK3 step from the saved state -> fields, Gⁿ, G⁻, pNHS"""
    for n, a in saved.items():
        model._field(n).set_parent(a)
    ocn.update_state(model, True)
    ocn.time_step(model, dt)
    names = _state_names(model)
    return [model._field(pre + n).parent() for pre in ("", "G", "M") for n in names] + [model._field("p").parent()]


def _stepped_the_same(ocn, model, twin, saved, dt, combo):
    """the default path, where the substep of stages 2 and 3 rides in the epilogue, against fused_epilogue = 0, where it is its own launch.
    Two models in lockstep, not one model stepped twice: on a Bounded z the pressure solver re-reads its previous solution in the singular
    column (ocn_poisson.h), which shifts the next one by round-off -- the two models have solved the same systems in the same order"""
    assert model.get_option("fuse_substep_active") == 1 and twin.get_option("fuse_substep_active") == 0, combo
    assert model.get_option("stokes_path") == 2 * model.get_option("stokes_drift") and twin.get_option("stokes_path") == twin.get_option("stokes_drift"), combo
    fused, plain = _step_from(ocn, model, saved, dt), _step_from(ocn, twin, saved, dt)
    assert all(np.all(np.isfinite(a)) for a in fused + plain), combo
    worst = max(float(np.abs(a - b).max()) for a, b in zip(fused, plain))
    assert _same(fused, plain), (combo, worst)
    # the step moved the fields: the comparison is not one of untouched arrays
    assert not np.array_equal(fused[0], saved["u"]), combo
    for n, a in saved.items():
        model._field(n).set_parent(a)


@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("ntr", [0, 1, 2, 3])
def test_every_physics_combination_takes_the_same_bits_on_all_three_paths(ocn, arch, ntr, closure):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    grid, model = _model(ocn, arch, ntr)
    _, twin = _model(ocn, arch, ntr)              # the same setters in lockstep, fused_epilogue = 0 throughout: it only steps (_stepped_the_same)
    twin.set_option("fused_epilogue", 0)
    both = (model, twin)
    bare = _tendencies(ocn, model)
    assert all(np.all(np.isfinite(g)) for g in bare)
    for m in both:
        _set_closure(L, m, closure, ntr)
    has_closure, vi = closure != "none", closure == "scalar_vi"
    metrics = R.Metrics.of_grid(grid)
    tables = order_one_stokes_drift(ocn).tables(grid)
    assert all(np.all(t != 0.0) and 0.01 < np.abs(t).max() < 1.0 for t in tables)          # all of ∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ act at every level
    saved, dt = _save(model), 0.05 / grid.Nx
    visited, coriolis, walk = set(), 0, 0
    for tilt in (0, 1):
        for m in both:
            if tilt:
                assert L.ocn_model_set_gravity_unit_vector(m.handle, 1, *GVEC) == 0
            else:
                assert L.ocn_model_set_gravity_unit_vector(m.handle, 0, 0.0, 0.0, 0.0) == 0
        for buoyancy in (0, 1, 2)[:min(ntr, 2) + 1]:
            for m in both:
                _set_buoyancy(L, m, buoyancy)
            for entry, kind in enumerate(WALKS[walk % 2]):
                for m in both:
                    _set_coriolis(L, m, kind, coriolis)
                visited.add((coriolis, kind))
                coriolis = kind
                combo = (ntr, closure, "tilt" if tilt else "vertical", buoyancy, coriolis)
                tilted = bool(tilt and buoyancy)
                march = has_closure and not vi and ntr <= 2 and coriolis != 2 and not tilted
                got = {k: model.get_option(k) for k in ("epilogue_march_active", "coriolis_kind", "tilted_gravity", "vertically_implicit")}
                want = {"epilogue_march_active": int(march), "coriolis_kind": coriolis, "tilted_gravity": int(tilted), "vertically_implicit": int(vi)}
                assert got == want, combo
                default = _tendencies(ocn, model)
                model.set_option("epilogue_march", 0)
                assert model.get_option("epilogue_march_active") == 0
                per_value = _tendencies(ocn, model)
                model.set_option("epilogue_march", 1)
                model.set_option("fused_epilogue", 0)
                assert model.get_option("epilogue_march_active") == 0
                standalone = _tendencies(ocn, model)
                model.set_option("fused_epilogue", 1)
                assert all(np.all(np.isfinite(g)) for g in default + per_value + standalone), combo
                worst = max(float(np.abs(a - b).max()) for other in (per_value, standalone) for a, b in zip(default, other))
                assert _same(default, per_value) and _same(default, standalone), (combo, worst)
                # the terms that are on, by the fields they reach: Coriolis and the hydrostatic gradient u and v (a Cartesian rotation
                # vector w too), a closure every field; with none on, the advective tendency itself
                changed = [not np.array_equal(a, b) for a, b in zip(default, bare)]
                if has_closure:
                    assert all(changed), combo
                elif coriolis or buoyancy:
                    assert changed[0] and changed[1] and changed[2] == (coriolis == 2) and not any(changed[3:]), combo
                else:
                    assert not any(changed), combo
                stepping = entry in (1, 3)
                if stepping and march:                # the marching epilogue with the substep riding along
                    _stepped_the_same(ocn, model, twin, saved, dt, combo + ("no drift",))
                # the STOKES instantiation of the same coordinates: G == the restatement's (G0 + curl) + ∂t, bit for bit
                U = {n: model._field(n).parent() for n in "uvw"}
                for m in both:
                    _set_drift(L, m, tables)
                got = {k: model.get_option(k) for k in ("stokes_drift", "stokes_path", "epilogue_march_active")}
                assert got == {"stokes_drift": 1, "stokes_path": 2, "epilogue_march_active": 0}, combo
                with_drift = _tendencies(ocn, model)
                model.set_option("fused_epilogue", 0)
                assert model.get_option("stokes_path") == 1, combo
                drift_standalone = _tendencies(ocn, model)
                model.set_option("fused_epilogue", 1)
                want = S.add_stokes_drift(metrics, tables, U, {n: default[q].copy(order="F") for q, n in enumerate("uvw")})
                assert all(np.all(np.isfinite(g)) for g in with_drift + drift_standalone), combo
                for q, n in enumerate("uvw"):
                    assert np.array_equal(with_drift[q], want[n]), (combo, "G" + n, float(np.abs(with_drift[q] - want[n]).max()))
                    assert not np.array_equal(with_drift[q], default[q]), (combo, "G" + n)
                assert _same(with_drift[3:], default[3:]), combo
                worst = max(float(np.abs(a - b).max()) for a, b in zip(with_drift, drift_standalone))
                assert _same(with_drift, drift_standalone), (combo, worst)
                if stepping:
                    _stepped_the_same(ocn, model, twin, saved, dt, combo + ("drift",))
                for m in both:
                    _set_drift(L, m, None)
                got = {k: model.get_option(k) for k in ("stokes_drift", "stokes_path", "epilogue_march_active")}
                assert got == {"stokes_drift": 0, "stokes_path": 0, "epilogue_march_active": int(march)}, combo
                assert _same(_tendencies(ocn, model), default), combo
            walk += 1
    # every replacement of one Coriolis by another (or by nothing) was made (without tracers: one walk per gravity vector, both kinds)
    assert visited == {(0, 1), (1, 2), (2, 1), (1, 0), (0, 2), (2, 0)}
    model.close()
    twin.close()


def test_set_closure_replaces_an_eddy_viscosity_closure(ocn, arch):
    """ocn_model_set_amd, then ocn_model_set_closure(nu != 0): the ScalarDiffusivity REPLACES the AMD closure. The fused and the stand-alone
    paths agree (and equal a model that only ever had the ScalarDiffusivity), "nu_e" answers OCN_ESTATE, and ocn_model_set_closure(0, NULL)
    afterwards leaves "fuse_substep_active" as on a model that never had a closure.

    This case documents a deliberate change and cannot pass on the commit before it: there ocn_model_set_closure left the AMD closure in
    place, the fused epilogue then ran the AMD terms alone and the stand-alone kernels the ScalarDiffusivity followed by AMD."""
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    ntr = 1
    grid, model = _model(ocn, arch, ntr)
    never = model.get_option("fuse_substep_active")
    bare = _tendencies(ocn, model)
    _set_closure(L, model, "amd", ntr)
    p, loc = C.c_void_p(), (C.c_int * 3)()
    assert L.ocn_model_field(model.handle, b"nu_e", C.byref(p), loc) == 0
    amd = _tendencies(ocn, model)
    _set_closure(L, model, "scalar", ntr)
    assert L.ocn_model_field(model.handle, b"nu_e", C.byref(p), loc) == OCN_ESTATE
    assert model.get_option("epilogue_march_active") == 1
    fused = _tendencies(ocn, model)
    model.set_option("fused_epilogue", 0)
    standalone = _tendencies(ocn, model)
    model.set_option("fused_epilogue", 1)
    _, scalar_only = _model(ocn, arch, ntr)
    _set_closure(L, scalar_only, "scalar", ntr)
    want = _tendencies(ocn, scalar_only)
    assert all(np.all(np.isfinite(g)) for g in fused + standalone)
    assert _same(fused, standalone) and _same(fused, want)
    assert not any(np.array_equal(a, b) for a, b in zip(fused, amd)) and not any(np.array_equal(a, b) for a, b in zip(fused, bare))
    # all zeros: closure = nothing, whatever the closure was
    assert L.ocn_model_set_closure(model.handle, 0.0, None) == 0
    assert model.get_option("fuse_substep_active") == never and model.get_option("epilogue_march_active") == 0
    assert L.ocn_model_field(model.handle, b"nu_e", C.byref(p), loc) == OCN_ESTATE
    assert _same(_tendencies(ocn, model), bare)
    model.close()
    scalar_only.close()
