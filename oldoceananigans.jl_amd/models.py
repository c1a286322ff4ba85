"""NonhydrostaticModel + RK3 time stepping (reference: src/Models/NonhydrostaticModels/nonhydrostatic_model.jl:115-244,
src/TimeSteppers/runge_kutta_3.jl:93-170). The whole time-step runs inside libocn_mi355x.so (`ocn_model_time_step`);
this module is the host-side mirror of the reference's API."""
import ctypes as C
import weakref
from collections import namedtuple

from . import _lib
from .advection import WENO
from .fields import Field
from .grids import Center, Face


class Clock:
    """TimeSteppers/clock.jl:39-45 (read-only view of the library's clock). Holds a WEAK reference to its model: no reference
    cycle, so a model is destroyed (and its FFT plans released) as soon as the last user reference goes away."""

    def __init__(self, model):
        self._model = weakref.ref(model)

    def _get(self):
        model = self._model()
        if model is None or model.handle is None:
            raise _lib.OcnError("the model of this clock has been destroyed")
        t, it, st, ldt, lsdt = C.c_double(), C.c_int64(), C.c_int(), C.c_double(), C.c_double()
        _lib.check(_lib.lib().ocn_model_clock(model.handle, C.byref(t), C.byref(it), C.byref(st), C.byref(ldt),
                                              C.byref(lsdt)))
        return t.value, it.value, st.value, ldt.value, lsdt.value

    time = property(lambda self: self._get()[0])
    iteration = property(lambda self: self._get()[1])
    stage = property(lambda self: self._get()[2])
    last_Δt = property(lambda self: self._get()[3])
    last_stage_Δt = property(lambda self: self._get()[4])


class NonhydrostaticModel:
    """NonhydrostaticModel(; grid, advection=WENO(), tracers=(:T, :S), timestepper=:RungeKutta3, coriolis, buoyancy, closure, forcing,
    boundary_conditions, background_fields, stokes_drift, particles); BASELINE.json benchmarks the configuration with all of them = nothing. `forcing`
    takes the closure-free forcings of forcings.py (Relaxation, Forcing(array), MultipleForcings / tuples); `background_fields` a dict or a
    BackgroundFields of time-independent backgrounds (background_fields.py); `stokes_drift` a time-independent UniformStokesDrift
    (stokes_drifts.py); `particles` a LagrangianParticles (particles.py): model.particles is then the model's own bound copy."""

    def __init__(self, grid, advection=None, tracers=("T", "S"), timestepper="RungeKutta3", buoyancy=None, coriolis=None,
                 closure=None, forcing=None, boundary_conditions=None, background_fields=None, stokes_drift=None, particles=None):
        if advection is None:
            advection = WENO()
        if not (isinstance(advection, WENO) and advection.order == 5 and advection.bounds is None):
            raise NotImplementedError("only advection = WENO(order=5) without bounds is on the accelerated hot path")
        timestepper = str(timestepper).lstrip(":")
        if timestepper not in ("RungeKutta3", "QuasiAdamsBashforth2"):
            raise NotImplementedError("timestepper must be :RungeKutta3 (hot path) or :QuasiAdamsBashforth2 (SURVEY.md 8f.1)")
        self.timestepper, self.χ = timestepper, 0.1          # QuasiAdamsBashforth2TimeStepper(χ = 0.1)
        from .buoyancy import BuoyancyForce, BuoyancyTracer, ConstantCartesianCoriolis, FPlane, SeawaterBuoyancy
        if coriolis is not None and not isinstance(coriolis, (FPlane, ConstantCartesianCoriolis)):
            raise NotImplementedError("coriolis must be nothing, FPlane(f) or ConstantCartesianCoriolis(fx, fy, fz)")
        self.coriolis = coriolis
        # a bare formulation is BuoyancyForce(formulation) with NegativeZDirection() (regularize_buoyancy, buoyancy_force.jl:74-75): the
        # calls below are then the ones a bare formulation always made
        force = buoyancy if isinstance(buoyancy, BuoyancyForce) else None
        formulation = force.formulation if force is not None else buoyancy
        if formulation is not None and not isinstance(formulation, (BuoyancyTracer, SeawaterBuoyancy)):
            raise NotImplementedError("buoyancy must be nothing, BuoyancyTracer(), SeawaterBuoyancy(LinearEquationOfState) or a BuoyancyForce of one")
        self.buoyancy = buoyancy
        tilted = force is not None and force.tilted
        from . import immersed_boundaries as _immersed
        immersed = _immersed.is_immersed(grid)
        if immersed:                                     # refused here, before any handle exists
            _immersed.validate_model(grid, closure, force, coriolis, background_fields, stokes_drift, particles, boundary_conditions)
        if hasattr(grid, "local") and (tilted or isinstance(coriolis, ConstantCartesianCoriolis)):
            raise NotImplementedError("ConstantCartesianCoriolis and BuoyancyForce(gravity_unit_vector) are not served on partitioned grids")
        from . import stokes_drifts as _stokes
        _stokes.validate_stokes_drift(stokes_drift, grid)
        from .closures import AnisotropicMinimumDissipation, ScalarDiffusivity, Smagorinsky
        if closure is not None and not isinstance(closure, (ScalarDiffusivity, AnisotropicMinimumDissipation, Smagorinsky)):
            raise NotImplementedError("only closure = nothing | ScalarDiffusivity(ν, κ) | AnisotropicMinimumDissipation(C, Cν, Cκ) | "
                                      "Smagorinsky(coefficient, Pr) | SmagorinskyLilly(C, Cb, Pr) is on the accelerated path (SURVEY.md 8f)")
        if getattr(closure, "dynamic", False) and hasattr(grid, "local"):
            raise NotImplementedError("Smagorinsky with a DynamicCoefficient is not served on partitioned grids")
        from .closures import is_vertically_implicit
        from .grids import Bounded
        if is_vertically_implicit(closure) and getattr(grid, "local", grid).topology[2] is not Bounded:
            # implicit_diffusion_solver (vertically_implicit_diffusion_solver.jl:149-153)
            raise ValueError("VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.")
        self.closure = closure
        # OpenBoundaryCondition(value; scheme = PerturbationAdvection(...)): refused here where the reference has no method for it
        from .boundary_conditions import validate_open_boundary_schemes
        validate_open_boundary_schemes(boundary_conditions, grid)
        # FluxBoundaryCondition(func, ...): refused here on partitioned grids and on diffusivity fields
        from .boundary_conditions import validate_boundary_functions
        validate_boundary_functions(boundary_conditions, grid)
        # "Adjust advection scheme to be valid on a particular grid size" and "Adjust halos when the advection scheme or turbulence
        # closure requires it" (nonhydrostatic_model.jl:176-184). The library derives the same per-direction schemes from the grid
        # size (ocn_grid_create), so only the descriptor and the halo are settled here.
        from .advection import adapt_advection_order, inflate_halo_size
        from .grids import with_halo
        advection = adapt_advection_order(advection, grid)
        required = inflate_halo_size(*grid.halo_size, grid, advection, closure)
        if any(u < r for u, r in zip(grid.halo_size, required)):
            import warnings
            note = ("Note that an ImmersedBoundaryGrid requires an extra halo point in all non-flat directions compared to a non-immersed "
                    "boundary grid. ") if immersed else ""             # (nonhydrostatic_model.jl:252-256)
            warnings.warn(f"Inflating model grid halo size to {required} and recreating grid. {note}The model grid will be different from the "
                          f"input grid. To avoid this warning, pass halo={required} when constructing the grid.")
            grid = with_halo(required, grid)
        self.grid, self.advection = grid, advection
        self.tracer_names = tuple(str(t) for t in (tracers if isinstance(tracers, (tuple, list)) else (tracers,)))
        # forcing = (u = ..., T = ...,) (model_forcing.jl): regularised before the handle exists, so a refused forcing costs no device memory
        from . import forcings as _forcings
        locations = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}
        locations.update({t: (Center, Center, Center) for t in self.tracer_names})
        self._forcing_terms = _forcings.model_forcing(getattr(grid, "local", grid), locations, forcing)
        _forcings.refuse_functions_on_partitions(self._forcing_terms, grid)
        self.forcing = dict(forcing or {})
        # background_fields = (u = U, b = B) (nonhydrostatic_model.jl:196-197): regularised on the host for the same reason
        from . import background_fields as _background
        self.background_fields = _background.regularize_background_fields(background_fields, self.tracer_names, grid, 0.0)
        self._has_background = self.background_fields is not None
        if not self._has_background:                     # BackgroundFields of ZeroFields: every entry None
            self.background_fields = _background.empty_background_fields(self.tracer_names)
        # stokes_drift = UniformStokesDrift(...) (nonhydrostatic_model.jl:115-130): its per-level tables, settled on the host as well
        self.stokes_drift = stokes_drift
        self._stokes_tables = _stokes.regularize_stokes_drift(stokes_drift, grid, 0.0)
        # particles = LagrangianParticles(...) (nonhydrostatic_model.jl:115-130): validated here, uploaded once the closure is set
        from . import particles as _particles
        from .closures import AnisotropicMinimumDissipation as _AMD, Smagorinsky as _Smag
        tracked = _particles.validate_particles(particles, grid, self.tracer_names, buoyancy is not None, isinstance(closure, (_AMD, _Smag)))
        self.particles = None
        if immersed:
            # nonhydrostatic_pressure_solver(arch, ibg::IBGWithFFTSolver) (NonhydrostaticModels.jl:42-58): the underlying grid's solver
            import warnings
            warnings.warn(_immersed.FFT_WARNING)
        self.handle = self._create_handle(grid, len(self.tracer_names))
        self.clock = Clock(self)
        V = namedtuple("Velocities", "u v w")
        self.velocities = V(self._field("u"), self._field("v"), self._field("w"))
        T = namedtuple("Tracers", self.tracer_names) if self.tracer_names else tuple
        self.tracers = T(*[self._field("c%d" % n) for n in range(len(self.tracer_names))])
        if buoyancy is not None:
            # validate_buoyancy / tracernames (nonhydrostatic_model.jl:166-170): the formulation's tracers must exist
            missing = [t for t in buoyancy.required_tracers if t not in self.tracer_names]
            if missing:
                raise ValueError(f"{buoyancy!r} requires the tracers {missing}")
            idx = [self.tracer_names.index(t) for t in buoyancy.required_tracers]
            if isinstance(formulation, BuoyancyTracer):
                _lib.check(_lib.lib().ocn_model_set_buoyancy(self.handle, 1, idx[0], 0, 0.0, 0.0, 0.0))
            else:
                e = formulation.equation_of_state
                _lib.check(_lib.lib().ocn_model_set_buoyancy(self.handle, 2, idx[0], idx[1], formulation.gravitational_acceleration,
                                                             e.thermal_expansion, e.haline_contraction))
            if tilted:
                _lib.check(_lib.lib().ocn_model_set_gravity_unit_vector(self.handle, 1, *force.gravity_unit_vector))
            P = namedtuple("Pressures", "pNHS pHY")          # pHY′: the hydrostatic pressure anomaly (nonhydrostatic_model.jl:144-158)
            self.pressures = P(self._field("p"), self._field("pHY"))
        else:
            P = namedtuple("Pressures", "pNHS")
            self.pressures = P(self._field("p"))
        if isinstance(coriolis, ConstantCartesianCoriolis):
            _lib.check(_lib.lib().ocn_model_set_cartesian_coriolis(self.handle, 1, coriolis.fx, coriolis.fy, coriolis.fz))
        elif coriolis is not None:
            _lib.check(_lib.lib().ocn_model_set_coriolis(self.handle, 1, coriolis.f))
        self.diffusivity_fields = None
        if isinstance(closure, AnisotropicMinimumDissipation):
            self._kappa, kp = closure.Ckappa_array(self.tracer_names)
            _lib.check(_lib.lib().ocn_model_set_amd(self.handle, closure.Cν, kp))
            # build_diffusivity_fields (anisotropic_minimum_dissipation.jl:339-352). Python normalises identifiers (NFKC): the
            # attribute written `.νₑ` in source is looked up as "νe", so the tuple's field names are the normalised spellings
            import unicodedata
            D = namedtuple("DiffusivityFields", [unicodedata.normalize("NFKC", n) for n in ("νₑ", "κₑ")])
            K = namedtuple("EddyDiffusivities", self.tracer_names) if self.tracer_names else tuple
            self.diffusivity_fields = D(self._field("nu_e"), K(*[self._field("kappa_e%d" % n) for n in range(len(self.tracer_names))]))
        elif isinstance(closure, Smagorinsky):
            self._kappa, pp = closure.Pr_array(self.tracer_names)
            import unicodedata
            if closure.dynamic:
                # allocate_coefficient_fields (dynamic_coefficient.jl:219-230, 332-345) merged behind νₑ (smagorinsky.jl:131-139). The
                # reference's names come first, NFKC-normalised as Python does with identifiers; ASCII aliases are properties beside them
                dc = closure.coefficient
                _lib.check(_lib.lib().ocn_model_set_dynamic_smagorinsky(self.handle, dc.averaging_mask, dc.minimum_numerator,
                                                                        dc.schedule.interval, dc.schedule.offset, pp))
                reduced = tuple(None if (dc.averaging_mask >> d) & 1 else Center for d in range(3))
                ccc = (Center, Center, Center)
                if dc.averaging_mask:
                    spec = [("Σ", "Sigma", ccc), ("Σ̄", "Sigma_bar", ccc), ("LM", "LM", ccc), ("MM", "MM", ccc),
                            ("𝒥ᴸᴹ", "J_LM", reduced), ("𝒥ᴹᴹ", "J_MM", reduced)]
                else:
                    spec = [("Σ", "Sigma", ccc), ("Σ̄", "Sigma_bar", ccc), ("𝒥ᴸᴹ", "J_LM", ccc), ("𝒥ᴹᴹ", "J_MM", ccc),
                            ("𝒥ᴸᴹ⁻", "J_LM_prev", ccc), ("𝒥ᴹᴹ⁻", "J_MM_prev", ccc)]
                self.diffusivity_fields = _dynamic_diffusivity_fields(self, [("νₑ", "nu_e", ccc)] + spec)
            else:
                _lib.check(_lib.lib().ocn_model_set_smagorinsky(self.handle, closure.coefficient, closure.Cb, int(closure.lilly), pp))
                # build_diffusivity_fields (smagorinsky.jl:131-139): νₑ only
                D = namedtuple("DiffusivityFields", [unicodedata.normalize("NFKC", "νₑ")])
                self.diffusivity_fields = D(self._field("nu_e"))
        elif closure is not None:
            self._kappa, kp = closure.kappa_array(self.tracer_names)
            _lib.check(_lib.lib().ocn_model_set_closure(self.handle, closure.ν, kp))
            if is_vertically_implicit(closure):
                _lib.check(_lib.lib().ocn_model_set_vertically_implicit(self.handle, 1))
        if self._stokes_tables is not None:
            dp = C.POINTER(C.c_double)
            _lib.check(_lib.lib().ocn_model_set_stokes_drift(self.handle, 1, *[t.ctypes.data_as(dp) for t in self._stokes_tables]))
        if self._has_background:
            _background.upload(self, self.background_fields)                  # borrowed by the library: the Fields are kept here
        self._forcing_keep = []                          # device arrays of Forcing(array): owned (numpy) or borrowed (Field)
        for name, terms in self._forcing_terms.items():
            _forcings.set_forcing(self.handle, ("u", "v", "w").index(name) if name in ("u", "v", "w") else 3 + self.tracer_names.index(name),
                                  terms, getattr(grid, "local", grid), self._forcing_keep, self._cname)
        # boundary_conditions = (u = FieldBoundaryConditions(top = FluxBoundaryCondition(Q)), ...) (nonhydrostatic_model.jl:
        # 163-190): constant Flux / Value / Gradient / Open conditions on Bounded sides
        self.boundary_conditions = dict(boundary_conditions or {})
        from .boundary_conditions import KINDS, SIDES
        import unicodedata
        targets = []                                     # (library field name, FieldBoundaryConditions)
        for name, fbcs in self.boundary_conditions.items():
            key = unicodedata.normalize("NFKC", name)
            if key in ("νe", "nu_e", "κe", "kappa_e"):
                # boundary_conditions = (νₑ = FieldBoundaryConditions(...), κₑ = (b = FieldBoundaryConditions(...),)): the diffusivity
                # fields of an LES closure (anisotropic_minimum_dissipation.jl:339-352)
                if self.diffusivity_fields is None:
                    raise ValueError(f"boundary conditions given for {name}, but the closure has no diffusivity fields")
                if key in ("νe", "nu_e"):
                    targets.append(("nu_e", fbcs))
                elif "κe" not in self.diffusivity_fields._fields:
                    raise ValueError(f"boundary conditions given for {name}, but the closure's diffusivity fields are νₑ only")
                else:
                    for tracer, tb in dict(fbcs).items():
                        if tracer not in self.tracer_names:
                            raise ValueError(f"κₑ boundary conditions given for {tracer}, which is not a tracer of the model")
                        targets.append(("kappa_e%d" % self.tracer_names.index(tracer), tb))
                continue
            if name not in ("u", "v", "w") + self.tracer_names:
                raise ValueError(f"boundary conditions given for {name}, which is not a velocity or tracer of the model")
            targets.append((self._cname(name), fbcs))
        self.boundary_functions = {}                     # (field name, side) -> RegularizedBoundaryFunction
        names = {self._cname(n): n for n in ("u", "v", "w") + self.tracer_names}
        for cname, fbcs in targets:
            for side, bc in fbcs.sides.items():
                if getattr(bc, "function", None) is not None:
                    # regularize_boundary_condition (continuous_boundary_function.jl:76-92): the function is recorded once, here
                    from .boundary_functions import RegularizedBoundaryFunction, program_array
                    if cname not in names:
                        raise NotImplementedError(f"a function-valued condition of the diffusivity field {cname} is not built")
                    rbf = RegularizedBoundaryFunction(bc.function, self.grid, locations[names[cname]], SIDES.index(side), tuple(names.values()))
                    program, n = program_array(rbf.program)
                    deps = (C.c_char_p * max(len(rbf.field_dependencies), 1))(*[self._cname(d).encode() for d in rbf.field_dependencies])
                    _lib.check(_lib.lib().ocn_model_set_flux_bc_function(self.handle, cname.encode(), SIDES.index(side), program, n, deps,
                                                                         len(rbf.field_dependencies)))
                    self.boundary_functions[(names[cname], side)] = rbf
                    continue
                if bc.linear is not None:
                    a, b, dep = bc.linear
                    _lib.check(_lib.lib().ocn_model_set_linear_flux_bc(self.handle, cname.encode(), SIDES.index(side), a, b,
                                                                       self._cname(dep).encode()))
                    continue
                if bc.array is not None:
                    from .boundary_conditions import _tangential_shape
                    dev = bc.device_array(_tangential_shape(self.grid, SIDES.index(side)))      # borrowed by the library: `bc` is kept
                    _lib.check(_lib.lib().ocn_model_set_boundary_condition_array(self.handle, cname.encode(), SIDES.index(side),
                                                                                 KINDS[bc.classification], dev))
                else:
                    _lib.check(_lib.lib().ocn_model_set_boundary_condition(self.handle, cname.encode(), SIDES.index(side),
                                                                           KINDS[bc.classification], bc.condition))
                if getattr(bc, "scheme", None) is not None:
                    _lib.check(_lib.lib().ocn_model_set_open_boundary_scheme(self.handle, cname.encode(), SIDES.index(side), 1,
                                                                             bc.scheme.inflow_timescale, bc.scheme.outflow_timescale))
        if particles is not None:
            self.particles = particles._bind(self, tracked)

    def _create_handle(self, grid, ntracers):
        h = C.c_void_p()
        _lib.check(_lib.lib().ocn_model_create(C.byref(h), grid.handle, ntracers))
        return h

    @property
    def architecture(self):
        return self.grid.architecture

    def _field(self, cname):
        p, loc = C.c_void_p(), (C.c_int * 3)()
        _lib.check(_lib.lib().ocn_model_field(self.handle, cname.encode(), C.byref(p), loc))
        return Field(tuple(Face if l else Center for l in loc), self.grid, data=p)   # a VIEW: valid while the model lives

    def tendency(self, name, previous=False):
        """timestepper.Gⁿ[name] / G⁻[name]; pointers are stable at time-step boundaries."""
        return self._field(("M" if previous else "G") + self._cname(name))

    def _cname(self, name):
        if name in ("u", "v", "w"):
            return name
        if name in self.tracer_names:
            return "c%d" % self.tracer_names.index(name)
        raise ValueError(f"name {name} not found in model.velocities or model.tracers.")

    def fields(self):
        d = dict(zip("uvw", self.velocities))
        d.update(dict(zip(self.tracer_names, self.tracers)))
        return d

    def set_option(self, key, value):
        """a tuning option of this model only (include/ocn_mi355x.h: ocn_set_option lists the keys); options read when the model is
        built raise OcnError here: set them with architectures.set_option before creating the model"""
        _lib.check(_lib.lib().ocn_model_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int()
        _lib.check(_lib.lib().ocn_model_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def boundary_function_values(self, name, side):
        """the array of the function-valued Flux condition name.side as the library last evaluated it: (Na, Nb) over the two tangential
        directions"""
        import numpy as np
        from .boundary_conditions import SIDES, _tangential_shape
        out = np.empty(_tangential_shape(self.grid, SIDES.index(side)), dtype=np.float64, order="F")
        _lib.check(_lib.lib().ocn_model_boundary_function_values(self.handle, self._cname(name).encode(), SIDES.index(side),
                                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def profile_read(self):
        """(total ms, count) of the event-timed tendency evaluations since the last read"""
        ms, n = C.c_double(), C.c_int()
        _lib.check(_lib.lib().ocn_model_profile_read(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        """release the model's device memory and FFT plans now (also called by the destructor)"""
        if getattr(self, "handle", None) is not None:
            _lib.lib().ocn_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dynamic_diffusivity_fields(model, spec):
    """the diffusivity fields of a dynamic Smagorinsky closure as a named tuple: per entry the reference's name, the library's name and the
    location (None along an averaged direction: one point, no halo). A name is spelt as Python spells the identifier (NFKC: 𝒥ᴸᴹ is JLM),
    the library's ASCII name where that is no identifier (𝒥ᴸᴹ⁻); the ASCII names are attributes as well"""
    import unicodedata
    names = []
    for reference, ascii_name, _ in spec:
        n = unicodedata.normalize("NFKC", reference)
        names.append(n if n.isidentifier() else ascii_name)
    base = namedtuple("DiffusivityFields", names)
    aliases = {a: q for q, ((_, a, _), n) in enumerate(zip(spec, names)) if a != n}
    D = type("DiffusivityFields", (base,), dict({a: property(lambda self, q=q: self[q]) for a, q in aliases.items()}, __slots__=()))
    fields = []
    for _, ascii_name, loc in spec:
        p = C.c_void_p()
        _lib.check(_lib.lib().ocn_model_field(model.handle, ascii_name.encode(), C.byref(p), None))
        fields.append(Field(loc, model.grid, data=p))
    return D(*fields)


def set_model(model, enforce_incompressibility=True, **kwargs):
    """set!(model; enforce_incompressibility=true, kwargs...) (set_nonhydrostatic_model.jl:33-60)"""
    flds = model.fields()
    for name, value in kwargs.items():
        if name not in flds:
            raise ValueError(f"name {name} not found in model.velocities or model.tracers.")
        flds[name].set(value)
    _lib.check(_lib.lib().ocn_model_set_finalize(model.handle, int(enforce_incompressibility)))


def update_state(model, compute_tendencies=True):
    """update_state!(model; compute_tendencies) (update_nonhydrostatic_model_state.jl:20-56)"""
    _lib.check(_lib.lib().ocn_model_update_state(model.handle, int(compute_tendencies)))


def time_step(model, Δt, euler=False):
    """time_step!(model, Δt) (runge_kutta_3.jl:93-170; quasi_adams_bashforth_2.jl:74-123 when the model's timestepper is
    :QuasiAdamsBashforth2 -- `euler` as in the reference)"""
    if getattr(model, "timestepper", "RungeKutta3") == "QuasiAdamsBashforth2":
        _lib.check(_lib.lib().ocn_model_time_step_ab2(model.handle, float(Δt), float(model.χ), int(euler)))
    else:
        _lib.check(_lib.lib().ocn_model_time_step(model.handle, float(Δt)))


def max_abs_divergence(model):
    if hasattr(model, "ctx") and hasattr(model, "max_abs_divergence"):       # partitioned model: global maximum
        return model.max_abs_divergence()
    v = C.c_double()
    _lib.check(_lib.lib().ocn_model_max_abs_divergence(model.handle, C.byref(v)))
    return v.value
