"""Raw kernel entry points on borrowed Fields: what `launch!(arch, grid, workspec, kernel!, args...)` runs for each
hot-path kernel of the reference."""
import ctypes as C

import numpy as np

from . import _lib
from .fields import _loc_array, _ptr_array


def _range(r):
    return None if r is None else (C.c_int * 6)(*[int(x) for x in r])


def compute_Gu(grid, u, v, w, Gu, kernel_parameters=None):
    _lib.check(_lib.lib().ocn_compute_Gu(grid.handle, u.data, v.data, w.data, Gu.data, _range(kernel_parameters)))


def compute_Gv(grid, u, v, w, Gv, kernel_parameters=None):
    _lib.check(_lib.lib().ocn_compute_Gv(grid.handle, u.data, v.data, w.data, Gv.data, _range(kernel_parameters)))


def compute_Gw(grid, u, v, w, Gw, kernel_parameters=None):
    _lib.check(_lib.lib().ocn_compute_Gw(grid.handle, u.data, v.data, w.data, Gw.data, _range(kernel_parameters)))


def compute_Gc(grid, u, v, w, c, Gc, kernel_parameters=None):
    _lib.check(_lib.lib().ocn_compute_Gc(grid.handle, u.data, v.data, w.data, c.data, Gc.data, _range(kernel_parameters)))


def compute_tendencies(grid, u, v, w, tracers, Gu, Gv, Gw, Gc, kernel_parameters=None):
    """compute_interior_tendency_contributions! as one fused flux-sharing pass"""
    tr = _ptr_array(tracers) if tracers else None
    gc = _ptr_array(Gc) if Gc else None
    _lib.check(_lib.lib().ocn_compute_tendencies(grid.handle, u.data, v.data, w.data, tr, len(tracers), Gu.data, Gv.data,
                                                 Gw.data, gc, _range(kernel_parameters)))


def compute_advective_tendency(grid, ua, va, wa, psi, which, G, kernel_parameters=None, accumulate=False):
    """G = -div(advection, (ua, va, wa), psi), or G = G - div(...) with `accumulate`: one advection term with the advecting velocities apart
    from the advected field (a model with background_fields evaluates two per field); which: "u" | "v" | "w" | "c" -- psi and G at that
    field's location"""
    _lib.check(_lib.lib().ocn_compute_advective_tendency(grid.handle, ua.data, va.data, wa.data, psi.data, "uvwc".index(which), G.data,
                                                         _range(kernel_parameters), int(accumulate)))


def sum_parent(grid, a, b, out):
    """out = a + b over the whole parent array (the total velocities u + Ū of a model with background fields)"""
    _lib.check(_lib.lib().ocn_sum_parent(grid.handle, a.data, b.data, _lib.i3(out.loc_codes), out.data))


# ---------------------------------------------------------------------------------------------------------------------
# diagnostics: one operation node (a Field or a BinaryOperation, diagnostics.py) evaluated, reduced or accumulated on the device
# ---------------------------------------------------------------------------------------------------------------------
def compute_operation(grid, operand, out):
    """_compute!(data, operand) (computed_field.jl:100-103): out[i, j, k] = operand[i, j, k] over the interior of `out`"""
    from .diagnostics import operand_struct
    _lib.check(_lib.lib().ocn_compute_operation(grid.handle, C.byref(operand_struct(operand)), out.data))


def reduce_operation(grid, operand, kind, dims, use_metric, absolute, out):
    """sum! / maximum! / minimum! / average! of the operand over the 1-based directions `dims` into the reduced field `out`; kind: "sum" |
    "maximum" | "minimum" | "average"; use_metric: the summand is operand * metric (Integral; Average over a stretched z)"""
    from .diagnostics import _KIND_CODE, dims_mask, operand_struct
    _lib.check(_lib.lib().ocn_reduce_operation(grid.handle, C.byref(operand_struct(operand)), _KIND_CODE[kind], dims_mask(dims), int(use_metric),
                                               int(absolute), out.data))


def accumulate_operation(grid, operand, dim, reverse, use_metric, out):
    """cumsum! / reverse_cumsum! of the operand along the 1-based direction `dim` into `out`; use_metric: operand * Δ (CumulativeIntegral)"""
    from .diagnostics import operand_struct
    _lib.check(_lib.lib().ocn_accumulate_operation(grid.handle, C.byref(operand_struct(operand)), int(dim) - 1, int(reverse), int(use_metric),
                                                   out.data))


def _stencil_struct(operand):
    """the ocn_stencil_operand_t of a Field, an operation (lowered by diagnostics.lower) or an operators.StencilProgram, with what it
    points to (pass it while both exist)"""
    from .diagnostics import lower
    from .operators import StencilProgram, program_array
    st = operand if isinstance(operand, StencilProgram) else lower(operand)
    if getattr(st, "_struct", None) is not None:              # the program is packed once; the device pointers are read every time
        s, keep = st._struct
        for q, f in enumerate(st.fields):
            keep[1][q] = f.data
        return st._struct
    s = _lib.StencilOperand()
    arr, s.n = program_array(st.program)
    s.program = arr
    ptrs = _ptr_array(st.fields) if st.fields else None
    locs = (C.c_int * (3 * max(len(st.fields), 1)))(*[c for f in st.fields for c in f.loc_codes])
    s.args, s.arg_locs, s.nargs = ptrs, locs, len(st.fields)
    s.loc[:] = [l.code for l in st.location]
    st._struct = (s, (arr, ptrs, locs))
    return st._struct


def compute_stencil(grid, operand, out):
    """_compute!(data, operand) of a stencil program -- a KernelFunctionOperation, a Derivative, a UnaryOperation, or ANY operand (a Field,
    a one-node BinaryOperation) forced through the interpreter: out[i, j, k] = operand[i, j, k] over the interior of `out`"""
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_compute_stencil(grid.handle, C.byref(s), out.data))


def reduce_stencil(grid, operand, kind, dims, use_metric, absolute, out):
    """reduce_operation with the operand as a stencil program: the same kernels, the interpreter as the evaluator"""
    from .diagnostics import _KIND_CODE, dims_mask
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_reduce_stencil(grid.handle, C.byref(s), _KIND_CODE[kind], dims_mask(dims), int(use_metric), int(absolute), out.data))


def accumulate_stencil(grid, operand, dim, reverse, use_metric, out):
    """accumulate_operation with the operand as a stencil program"""
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_accumulate_stencil(grid.handle, C.byref(s), int(dim) - 1, int(reverse), int(use_metric), out.data))


# ---------------------------------------------------------------------------------------------------------------------
# time averages: the six calls above with the fold of accumulate_result! (OutputWriters/windowed_time_average.jl:216-230) at the store.
# times: (T_previous, Δt, T_current, first) -- first: the first sample of a window, `result` is not read
# ---------------------------------------------------------------------------------------------------------------------
def _time_fold(times):
    T_previous, Δt, T_current, first = times
    return C.byref(_lib.TimeFold(float(T_previous), float(Δt), float(T_current), int(bool(first))))


def time_average_operation(grid, operand, times, result):
    """result = (result * T_previous + operand * Δt) / T_current: a Field over its whole parent array, halos included; a BinaryOperation
    over the interior of its location"""
    from .diagnostics import operand_struct
    _lib.check(_lib.lib().ocn_time_average_operation(grid.handle, C.byref(operand_struct(operand)), _time_fold(times), result.data))


def time_average_parent(field, times, result):
    """the fold of a materialised field of any shape (a reduced field has no operand form) over its whole parent array"""
    if field.shape != result.shape:
        raise ValueError(f"parent shape {field.shape} != {result.shape}")
    _lib.check(_lib.lib().ocn_time_average_parent(field.data, field.nbytes // 8, _time_fold(times), result.data))


def time_average_stencil(grid, operand, times, result):
    """time_average_operation with the operand as a stencil program, over the interior of its location"""
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_time_average_stencil(grid.handle, C.byref(s), _time_fold(times), result.data))


def time_average_reduce_operation(grid, operand, kind, dims, use_metric, absolute, times, result):
    """the fold of what reduce_operation would write, into the reduced field `result`"""
    from .diagnostics import _KIND_CODE, dims_mask, operand_struct
    _lib.check(_lib.lib().ocn_time_average_reduce_operation(grid.handle, C.byref(operand_struct(operand)), _KIND_CODE[kind], dims_mask(dims),
                                                            int(use_metric), int(absolute), _time_fold(times), result.data))


def time_average_reduce_stencil(grid, operand, kind, dims, use_metric, absolute, times, result):
    from .diagnostics import _KIND_CODE, dims_mask
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_time_average_reduce_stencil(grid.handle, C.byref(s), _KIND_CODE[kind], dims_mask(dims), int(use_metric), int(absolute),
                                                          _time_fold(times), result.data))


def time_average_accumulate_operation(grid, operand, dim, reverse, use_metric, times, result):
    """the fold of what accumulate_operation would write: the running sum stays in registers"""
    from .diagnostics import operand_struct
    _lib.check(_lib.lib().ocn_time_average_accumulate_operation(grid.handle, C.byref(operand_struct(operand)), int(dim) - 1, int(reverse),
                                                                int(use_metric), _time_fold(times), result.data))


def time_average_accumulate_stencil(grid, operand, dim, reverse, use_metric, times, result):
    s, keep = _stencil_struct(operand)
    _lib.check(_lib.lib().ocn_time_average_accumulate_stencil(grid.handle, C.byref(s), int(dim) - 1, int(reverse), int(use_metric),
                                                              _time_fold(times), result.data))


def evaluate_boundary_function(grid, program, loc, side, deps, time, out=None):
    """getbc of a traced boundary function (boundary_functions.py: a list of instruction tuples (op, a, b, c, imm)) at every point of
    `side` ("west" .. "top" or 0..5) for a condition of a field at `loc`: `deps` are Fields with current halos, one per dependency slot;
    returns the host array (Na, Nb). `out`: a device pointer to evaluate into instead (then nothing is copied back)"""
    from .boundary_conditions import SIDES, _tangential_shape
    from .boundary_functions import program_array
    side = SIDES.index(side) if isinstance(side, str) else int(side)
    codes = [0 if l is None else l.code for l in loc]
    deps = list(deps)
    ptrs = _ptr_array(deps) if deps else None
    locs = _loc_array(deps) if deps else None
    arr, n = program_array(program)
    shape = _tangential_shape(grid, side) if 0 <= side <= 5 else (1, 1)
    dev = out
    if out is None:
        dev = C.c_void_p()
        _lib.check(_lib.lib().ocn_malloc(C.byref(dev), 8 * shape[0] * shape[1]))
    try:
        _lib.check(_lib.lib().ocn_evaluate_boundary_function(grid.handle, arr, n, _lib.i3(codes), side, ptrs, locs, len(deps), float(time), dev))
        if out is not None:
            return None
        host = np.empty(shape, dtype=np.float64, order="F")
        _lib.check(_lib.lib().ocn_memcpy_d2h(host.ctypes.data, dev, host.nbytes))
        return host
    finally:
        if out is None:
            _lib.lib().ocn_free(dev)


def evaluate_forcing_function(grid, program, loc, deps, time, hoist=True, out=None):
    """a traced function of (X..., t, deps...) (boundary_functions.trace with coordinates x / y / z = 0 / 1 / 2) at every interior point of
    a field at `loc`: what a function-valued forcing term adds. `deps` are Fields with current halos, one per dependency slot, each
    interpolated from its own location to `loc`. Returns the host interior array; with `out`, a Field at `loc`, evaluates into its interior
    and returns nothing -- Forcing(out) is borrowed, so this refreshes an arbitrary forcing between time-steps. hoist=False evaluates the
    whole program at every cell (the bits are the same)."""
    from .boundary_functions import program_array
    from .fields import Field
    deps = list(deps)
    ptrs = _ptr_array(deps) if deps else None
    locs = _loc_array(deps) if deps else None
    arr, n = program_array(program)
    field = out if out is not None else Field(loc, grid)
    _lib.check(_lib.lib().ocn_evaluate_forcing_function(grid.handle, arr, n, _lib.i3(field.loc_codes), ptrs, locs, len(deps), float(time),
                                                        int(bool(hoist)), field.data))
    return None if out is not None else field.interior()


def compute_tendencies_and_substep(grid, fields, Gn, next_fields, Gm, Δt, γ, ζ, kernel_parameters=None):
    """tendencies of all prognostic fields (u, v, w, tracers...) + the rk3_substep! of the next stage into `next_fields`"""
    _lib.check(_lib.lib().ocn_compute_tendencies_and_substep(
        grid.handle, _ptr_array(fields), len(fields) - 3, _ptr_array(Gn), _range(kernel_parameters), _ptr_array(next_fields),
        _ptr_array(Gm), float(Δt), float(γ), 0.0 if ζ is None else float(ζ), 0 if ζ is None else 1))


def compute_closure_tendencies(grid, fields, Gn, closure, tracer_names, kernel_parameters=None):
    """adds the ScalarDiffusivity terms (-∂ⱼτᵢⱼ, -∇·q) to tendencies that hold the advective part; fields = u, v, w, tracers..."""
    karr, kp = closure.kappa_array(tracer_names)
    tr, gc = fields[3:], Gn[3:]
    _lib.check(_lib.lib().ocn_compute_closure_tendencies(
        grid.handle, fields[0].data, fields[1].data, fields[2].data, _ptr_array(tr) if tr else None, len(tr), closure.ν, kp,
        Gn[0].data, Gn[1].data, Gn[2].data, _ptr_array(gc) if gc else None, _range(kernel_parameters)))


def compute_closure_tendencies_vertically_implicit(grid, fields, Gn, closure, tracer_names, kernel_parameters=None):
    """the explicit part of ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) (abstract_scalar_diffusivity_closure.jl:245-291),
    added to tendencies that hold the advective part; fields = u, v, w, tracers..."""
    karr, kp = closure.kappa_array(tracer_names)
    tr, gc = fields[3:], Gn[3:]
    _lib.check(_lib.lib().ocn_compute_closure_tendencies_vertically_implicit(
        grid.handle, fields[0].data, fields[1].data, fields[2].data, _ptr_array(tr) if tr else None, len(tr), closure.ν, kp,
        Gn[0].data, Gn[1].data, Gn[2].data, _ptr_array(gc) if gc else None, _range(kernel_parameters)))


def implicit_step(grid, field, coefficient, Δt, form=0):
    """implicit_step!(field, ...) for a constant coefficient (vertically_implicit_diffusion_solver.jl:189-213): the tridiagonal solve along
    z in place; form 0 is the reference-shaped kernel, the only form shipped"""
    _lib.check(_lib.lib().ocn_implicit_step_z(grid.handle, field.data, _lib.i3(field.loc_codes), float(coefficient), float(Δt), int(form)))


def compute_amd_diffusivities(grid, closure, tracer_names, fields, νₑ, κₑ, kernel_parameters=None):
    """compute_diffusivities!(…, closure::AnisotropicMinimumDissipation, …) over the interior; fields = u, v, w, tracers... with filled
    halos; fill the halos of νₑ, κₑ afterwards (fill_halo_regions)"""
    karr, kp = closure.Ckappa_array(tracer_names)
    tr = fields[3:]
    _lib.check(_lib.lib().ocn_compute_amd_diffusivities(
        grid.handle, closure.Cν, kp, fields[0].data, fields[1].data, fields[2].data, _ptr_array(tr) if tr else None, len(tr),
        νₑ.data, _ptr_array(κₑ) if κₑ else None, _range(kernel_parameters)))


def compute_closure_tendencies_field(grid, fields, Gn, νₑ, κₑ, kernel_parameters=None):
    """adds -∂ⱼτᵢⱼ, -∇·q with the coefficients read from the ccc arrays νₑ, κₑ[tracer] (halos filled)"""
    tr, gc = fields[3:], Gn[3:]
    _lib.check(_lib.lib().ocn_compute_closure_tendencies_field(
        grid.handle, fields[0].data, fields[1].data, fields[2].data, _ptr_array(tr) if tr else None, len(tr), νₑ.data,
        _ptr_array(κₑ) if κₑ else None, Gn[0].data, Gn[1].data, Gn[2].data, _ptr_array(gc) if gc else None, _range(kernel_parameters)))


def compute_smagorinsky_viscosity(grid, closure, buoyancy, tracers_by_name, u, v, w, νₑ, kernel_parameters=None):
    """compute_diffusivities!(…, closure::Smagorinsky, …) (smagorinsky.jl:113-127) over the interior or `kernel_parameters`; u, v, w and the
    buoyancy's tracers with filled halos; fill the halos of νₑ afterwards. buoyancy: None | BuoyancyTracer | linear SeawaterBuoyancy"""
    from .buoyancy import BuoyancyTracer
    kind, bT, S, g, α, β = 0, None, None, 0.0, 0.0, 0.0
    if isinstance(buoyancy, BuoyancyTracer):
        kind, bT = 1, tracers_by_name["b"].data
    elif buoyancy is not None:
        e = buoyancy.equation_of_state
        kind, bT, S = 2, tracers_by_name["T"].data, tracers_by_name["S"].data
        g, α, β = buoyancy.gravitational_acceleration, e.thermal_expansion, e.haline_contraction
    _lib.check(_lib.lib().ocn_compute_smagorinsky_viscosity(grid.handle, closure.coefficient, closure.Cb, int(closure.lilly), kind, bT, S, g, α, β,
                                                            u.data, v.data, w.data, νₑ.data, _range(kernel_parameters)))


def dynamic_coefficient_fields(grid, coefficient):
    """allocate_coefficient_fields (dynamic_coefficient.jl:219-230, 332-345) as a dict of zeroed Fields under the library's names: Sigma,
    Sigma_bar, J_LM, J_MM and LM, MM (directional; J_LM, J_MM reduced along the averaged directions) or J_LM_prev, J_MM_prev (Lagrangian)"""
    from .fields import CenterField, Field
    from .grids import Center
    mask = coefficient.averaging_mask
    reduced = tuple(None if (mask >> d) & 1 else Center for d in range(3))
    names = ("Sigma", "Sigma_bar", "LM", "MM") if mask else ("Sigma", "Sigma_bar", "J_LM", "J_MM", "J_LM_prev", "J_MM_prev")
    out = {n: CenterField(grid) for n in names}
    if mask:
        out["J_LM"], out["J_MM"] = Field(reduced, grid), Field(reduced, grid)
    for f in out.values():
        _lib.check(_lib.lib().ocn_memset_zero(f.data, f.nbytes))
    return out


def dynamic_smagorinsky_update(grid, coefficient, u, v, w, fields, Δt=0.0, initialising=True):
    """one update of the coefficient fields of Smagorinsky(coefficient = DynamicCoefficient(...)) -- compute_coefficient_fields! once the
    schedule has fired (dynamic_coefficient.jl:194-217, 292-330). u, v, w with filled halos; `fields` as dynamic_coefficient_fields makes
    them. Lagrangian averaging: `initialising` takes the first-time-step branch, else the averaging step over Δt"""
    ptr = lambda n: fields[n].data if n in fields else None                  # noqa: E731
    _lib.check(_lib.lib().ocn_dynamic_smagorinsky_update(grid.handle, u.data, v.data, w.data, coefficient.averaging_mask,
                                                         coefficient.minimum_numerator, float(Δt), int(bool(initialising)), ptr("Sigma"),
                                                         ptr("Sigma_bar"), ptr("LM"), ptr("MM"), ptr("J_LM"), ptr("J_MM"), ptr("J_LM_prev"),
                                                         ptr("J_MM_prev")))


def compute_dynamic_smagorinsky_viscosity(grid, coefficient, fields, u, v, w, νₑ):
    """_compute_smagorinsky_viscosity! with the coefficient of fields["J_LM"], fields["J_MM"] (smagorinsky.jl:92-106, dynamic_coefficient.jl:
    129-140) over the interior; fill the halos of νₑ afterwards"""
    _lib.check(_lib.lib().ocn_compute_dynamic_smagorinsky_viscosity(grid.handle, coefficient.averaging_mask, coefficient.minimum_numerator,
                                                                    fields["J_LM"].data, fields["J_MM"].data, u.data, v.data, w.data, νₑ.data))


def compute_closure_tendencies_smagorinsky(grid, fields, Gn, νₑ, closure, tracer_names, kernel_parameters=None):
    """adds -∂ⱼτᵢⱼ with νₑ and -∇·q with ℑ(νₑ) / Pr[tracer] (smagorinsky.jl:141-143); fields = u, v, w, tracers..., νₑ with filled halos"""
    parr, pp = closure.Pr_array(tracer_names)
    tr, gc = fields[3:], Gn[3:]
    _lib.check(_lib.lib().ocn_compute_closure_tendencies_smagorinsky(
        grid.handle, fields[0].data, fields[1].data, fields[2].data, _ptr_array(tr) if tr else None, len(tr), νₑ.data, pp,
        Gn[0].data, Gn[1].data, Gn[2].data, _ptr_array(gc) if gc else None, _range(kernel_parameters)))


def update_hydrostatic_pressure(grid, buoyancy, tracers_by_name, pHY):
    """update_hydrostatic_pressure! (update_hydrostatic_pressure.jl:12-49) for BuoyancyTracer | linear SeawaterBuoyancy"""
    from .buoyancy import BuoyancyTracer
    if isinstance(buoyancy, BuoyancyTracer):
        _lib.check(_lib.lib().ocn_update_hydrostatic_pressure(grid.handle, 1, tracers_by_name["b"].data, None, 0.0, 0.0, 0.0, pHY.data))
    else:
        e = buoyancy.equation_of_state
        _lib.check(_lib.lib().ocn_update_hydrostatic_pressure(grid.handle, 2, tracers_by_name["T"].data, tracers_by_name["S"].data,
                                                              buoyancy.gravitational_acceleration, e.thermal_expansion,
                                                              e.haline_contraction, pHY.data))


def add_fplane_coriolis(grid, f, u, v, Gu, Gv, kernel_parameters=None):
    """- x_f_cross_U, - y_f_cross_U of the u, v tendencies for coriolis = FPlane(f)"""
    _lib.check(_lib.lib().ocn_add_fplane_coriolis(grid.handle, float(f), u.data, v.data, Gu.data, Gv.data, _range(kernel_parameters)))


def add_cartesian_coriolis(grid, coriolis, u, v, w, Gu, Gv, Gw, kernel_parameters=None):
    """- x_f_cross_U, - y_f_cross_U, - z_f_cross_U of the u, v, w tendencies for coriolis = ConstantCartesianCoriolis(fx, fy, fz)"""
    _lib.check(_lib.lib().ocn_add_cartesian_coriolis(grid.handle, coriolis.fx, coriolis.fy, coriolis.fz, u.data, v.data, w.data, Gu.data, Gv.data,
                                                     Gw.data, _range(kernel_parameters)))


def add_stokes_drift(grid, stokes_drift, u, v, w, Gu, Gv, Gw, kernel_parameters=None, time=0.0):
    """+ x_curl_Uˢ_cross_U + ∂t_uˢ, + y_curl_Uˢ_cross_U + ∂t_vˢ, + z_curl_Uˢ_cross_U of the u, v, w tendencies for stokes_drift =
    UniformStokesDrift(...) evaluated at `time`, on tendencies that hold everything up to the closure term; kernel_parameters: one range for
    all three velocities (None: each field's own cells, the wall faces excluded)"""
    tables = stokes_drift.tables(grid, time)
    L = _lib.lib()
    block = C.c_void_p()
    _lib.check(L.ocn_malloc(C.byref(block), sum(t.nbytes for t in tables)))
    try:
        ptrs, off = [], 0
        for t in tables:                                 # the library reads DEVICE tables: one block, released after the launch has run
            ptrs.append(C.c_void_p(block.value + off))
            _lib.check(L.ocn_memcpy_h2d(ptrs[-1], t.ctypes.data_as(C.c_void_p), t.nbytes))
            off += t.nbytes
        r = _range(kernel_parameters)
        _lib.check(L.ocn_add_stokes_drift(grid.handle, *ptrs, u.data, v.data, w.data, Gu.data, Gv.data, Gw.data, r, r, r))
        _lib.check(L.ocn_sync())
    finally:
        L.ocn_free(block)


class _DeviceVectors:
    """host vectors in one device block for the length of a raw launch"""

    def __init__(self, arrays):
        self.arrays = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in arrays]
        self.block, self.ptrs = C.c_void_p(), []
        L = _lib.lib()
        _lib.check(L.ocn_malloc(C.byref(self.block), sum(a.nbytes for a in self.arrays if a is not None) + 8))
        off = 0
        try:
            for a in self.arrays:
                if a is None:
                    self.ptrs.append(None)
                    continue
                self.ptrs.append(C.c_void_p(self.block.value + off))
                if a.nbytes:
                    _lib.check(L.ocn_memcpy_h2d(self.ptrs[-1], a.ctypes.data_as(C.c_void_p), a.nbytes))
                off += a.nbytes
        except Exception:
            self.free()
            raise

    def read(self, q):
        out = np.empty_like(self.arrays[q])
        if out.nbytes:
            _lib.check(_lib.lib().ocn_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptrs[q], out.nbytes))
        return out

    def free(self):
        _lib.lib().ocn_free(self.block)


def interpolate(grid, field, x, y, z):
    """interpolate((x, y, z), field, location(field), grid) (Fields/interpolate.jl:272-336) at the points x[p], y[p], z[p] -> numpy array;
    the field with filled halos"""
    x = np.asarray(x, dtype=np.float64)
    d = _DeviceVectors([x, y, z, np.zeros_like(x)])
    try:
        _lib.check(_lib.lib().ocn_interpolate_at(grid.handle, x.size, *d.ptrs[:3], field.data, _lib.i3(field.loc_codes), d.ptrs[3]))
        return d.read(3)
    finally:
        d.free()


def advect_particles(grid, x, y, z, u, v, w, Δt, restitution=1.0, depths=None):
    """advect_lagrangian_particles! (lagrangian_particle_advection.jl:195-223; with depths: drogued_dynamics.jl:45-72) -> the new (x, y, z)"""
    x = np.asarray(x, dtype=np.float64)
    d = _DeviceVectors([x, y, z, depths])
    try:
        _lib.check(_lib.lib().ocn_advect_particles(grid.handle, x.size, *d.ptrs, float(restitution), float(Δt), u.data, v.data, w.data))
        return d.read(0), d.read(1), d.read(2)
    finally:
        d.free()


def _buoyancy_arguments(buoyancy, tracers_by_name):
    """(kind, b or T, S, g, α, β, ĝ) of a formulation or a BuoyancyForce"""
    from .buoyancy import BuoyancyForce, BuoyancyTracer
    ghat = (0.0, 0.0, 1.0)
    if isinstance(buoyancy, BuoyancyForce):
        if buoyancy.tilted:
            ghat = tuple(-c for c in buoyancy.gravity_unit_vector)              # ĝ = -gravity_unit_vector (buoyancy_force.jl:52-54)
        buoyancy = buoyancy.formulation
    if isinstance(buoyancy, BuoyancyTracer):
        return 1, tracers_by_name["b"].data, None, 0.0, 0.0, 0.0, ghat
    e = buoyancy.equation_of_state
    return (2, tracers_by_name["T"].data, tracers_by_name["S"].data, buoyancy.gravitational_acceleration, e.thermal_expansion,
            e.haline_contraction, ghat)


def add_buoyancy_acceleration(grid, buoyancy, tracers_by_name, Gu, Gv, kernel_parameters=None):
    """+ x_dot_g_b, + y_dot_g_b of the u, v tendencies for buoyancy = BuoyancyForce(formulation; gravity_unit_vector)"""
    kind, bT, S, g, α, β, ghat = _buoyancy_arguments(buoyancy, tracers_by_name)
    _lib.check(_lib.lib().ocn_add_buoyancy_acceleration(grid.handle, kind, bT, S, g, α, β, ghat[0], ghat[1], Gu.data, Gv.data,
                                                        _range(kernel_parameters)))


def update_hydrostatic_pressure_tilted(grid, buoyancy, tracers_by_name, pHY):
    """update_hydrostatic_pressure! with z_dot_g_b = ĝ_z ℑz(b) for buoyancy = BuoyancyForce(formulation; gravity_unit_vector)"""
    kind, bT, S, g, α, β, ghat = _buoyancy_arguments(buoyancy, tracers_by_name)
    _lib.check(_lib.lib().ocn_update_hydrostatic_pressure_tilted(grid.handle, kind, bT, S, g, α, β, ghat[2], pHY.data))


def add_hydrostatic_pressure_gradient(grid, pHY, Gu, Gv, kernel_parameters=None):
    """-∂x pHY′, -∂y pHY′ of the u, v tendencies"""
    _lib.check(_lib.lib().ocn_add_hydrostatic_pressure_gradient(grid.handle, pHY.data, Gu.data, Gv.data, _range(kernel_parameters)))


def rk3_substep(grid, fields, Gn, Gm, Δt, γ, ζ):
    """rk3_substep_field! over a tuple of fields (ζ = None -> first stage)"""
    _lib.check(_lib.lib().ocn_rk3_substep(grid.handle, _ptr_array(fields), _ptr_array(Gn), _ptr_array(Gm),
                                          _loc_array(fields), len(fields), float(Δt), float(γ),
                                          0.0 if ζ is None else float(ζ), 0 if ζ is None else 1))


def cache_tendencies(grid, Gm, Gn):
    _lib.check(_lib.lib().ocn_cache_tendencies(grid.handle, _ptr_array(Gm), _ptr_array(Gn), _loc_array(Gn), len(Gn)))


def make_pressure_correction(grid, u, v, w, p):
    _lib.check(_lib.lib().ocn_make_pressure_correction(grid.handle, u.data, v.data, w.data, p.data))


def divide_interior(grid, p, divisor):
    _lib.check(_lib.lib().ocn_divide_interior(grid.handle, p.data, float(divisor)))


# ---------------------------------------------------------------------------------------------------------------------
# open boundaries with a scheme, piece by piece (the model runs them inside its pressure step)
# ---------------------------------------------------------------------------------------------------------------------
def _side_conditions(grid, conditions):
    """{side: OpenBoundaryCondition} of the wall-normal velocities -> (ocn_bc_t[6], scheme mask)"""
    from .boundary_conditions import KINDS, SIDES, _tangential_shape
    arr, mask = (_lib.BC * 6)(), 0
    arr._keep = dict(conditions)                       # the device arrays live as long as the conditions
    for side, bc in conditions.items():
        q = SIDES.index(side)
        arr[q].kind, arr[q].value = KINDS[bc.classification], bc.condition
        if bc.array is not None:
            arr[q].array = bc.device_array(_tangential_shape(grid, q))
        if bc.scheme is not None:
            mask |= 1 << q
    return arr, mask


def step_open_boundary(field, side, condition, last_stage_Δt):
    """_fill_<side>_halo!(..., bc::PAOBC, ...) (perturbation_advection.jl:119-180) on the wall-normal velocity `field` for condition =
    OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)) and clock.last_stage_Δt"""
    from .boundary_conditions import SIDES, _tangential_shape
    q = SIDES.index(side)
    if condition.scheme is None:
        raise ValueError("step_open_boundary steps a condition with a scheme")
    dev = condition.device_array(_tangential_shape(field.grid, q)) if condition.array is not None else None
    _lib.check(_lib.lib().ocn_step_open_boundary(field.grid.handle, field.data, _lib.i3(field.loc_codes), q, condition.condition, dev,
                                                 condition.scheme.inflow_timescale, condition.scheme.outflow_timescale, float(last_stage_Δt)))


def open_boundary_mass_inflow(grid, u, v, w, sides):
    """Σ u Ax + Σ v Ay + Σ w Az over the left faces among `sides` minus the same over the right ones (open_boundary_mass_inflow,
    boundary_mass_fluxes.jl:181-198, every listed face integrated); synchronous"""
    from .boundary_conditions import SIDES
    mask = 0
    for s in sides:
        mask |= 1 << SIDES.index(s)
    out = C.c_double()
    _lib.check(_lib.lib().ocn_open_boundary_mass_inflow(grid.handle, u.data if u is not None else None, v.data if v is not None else None,
                                                        w.data if w is not None else None, mask, C.byref(out)))
    return out.value


def enforce_open_boundary_mass_conservation(grid, u, v, w, conditions):
    """enforce_open_boundary_mass_conservation! (boundary_mass_fluxes.jl:224-239) for conditions = {side: OpenBoundaryCondition} of the
    wall-normal velocities: the sides with a scheme are corrected, the imposed ones only enter the total"""
    arr, mask = _side_conditions(grid, conditions)
    _lib.check(_lib.lib().ocn_enforce_open_boundary_mass_conservation(grid.handle, u.data if u is not None else None,
                                                                      v.data if v is not None else None, w.data if w is not None else None,
                                                                      arr, mask))
