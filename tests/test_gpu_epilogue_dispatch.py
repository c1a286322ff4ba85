"""Which tendency epilogue a model runs, for every combination of physics the setters can reach: the selection is checked, not the kernels'
interiors (those are pinned by test_gpu_parity.py, test_gpu_tilted.py, test_gpu_smagorinsky.py, ...).

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
No combination is exempt: every one is bit-identical across the three paths."""
import ctypes as C

import numpy as np
import pytest

from helpers import smooth_state, tanh_faces

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


@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("ntr", [0, 1, 2, 3])
def test_every_physics_combination_takes_the_same_bits_on_all_three_paths(ocn, arch, ntr, closure):
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    grid, model = _model(ocn, arch, ntr)
    bare = _tendencies(ocn, model)
    assert all(np.all(np.isfinite(g)) for g in bare)
    _set_closure(L, model, closure, ntr)
    has_closure, vi = closure != "none", closure == "scalar_vi"
    visited, coriolis, walk = set(), 0, 0
    for tilt in (0, 1):
        if tilt:
            assert L.ocn_model_set_gravity_unit_vector(model.handle, 1, *GVEC) == 0
        else:
            assert L.ocn_model_set_gravity_unit_vector(model.handle, 0, 0.0, 0.0, 0.0) == 0
        for buoyancy in (0, 1, 2)[:min(ntr, 2) + 1]:
            _set_buoyancy(L, model, buoyancy)
            for kind in WALKS[walk % 2]:
                _set_coriolis(L, model, kind, coriolis)
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
            walk += 1
    # every replacement of one Coriolis by another (or by nothing) was made (without tracers: one walk per gravity vector, both kinds)
    assert visited == {(0, 1), (1, 2), (2, 1), (1, 0), (0, 2), (2, 0)}
    model.close()


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
