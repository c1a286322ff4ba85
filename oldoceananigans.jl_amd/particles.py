"""particles = LagrangianParticles(...) of the NonhydrostaticModel (reference: src/Models/LagrangianParticleTracking/
LagrangianParticleTracking.jl:41-161, drogued_dynamics.jl:34-72). Host-side descriptor; the particles of a model live in the library
(`ocn_model_set_particles`) and move inside `ocn_model_time_step`, one launch per step_lagrangian_particles!.

Served: x, y, z, restitution, custom properties, tracked_fields that name a model field, dynamics = DroguedParticleDynamics(depths).
Refused by name: any other callable `dynamics` (it cannot cross the C ABI, like callable forcings), tracked computed fields (the reference's
`speed = √(u² + v²)` needs AbstractOperations), partitioned grids (particles would have to migrate between ranks)."""
import copy
import ctypes as C
import weakref

import numpy as np

from . import _lib

MAX_TRACKED = 8           # OCN_MAX_TRACKED


def no_dynamics(*args):
    """no_dynamics(args...) = nothing (LagrangianParticleTracking.jl:49)"""
    return None


class DroguedParticleDynamics:
    """DroguedParticleDynamics(depths) (drogued_dynamics.jl:34-43): the particles keep their z -- where they measure -- and move in x and
    y with the velocity at `depths`, one depth per particle"""

    def __init__(self, depths):
        self.depths = np.ascontiguousarray(np.asarray(depths, dtype=np.float64))
        if self.depths.ndim != 1:
            raise ValueError("depths must be a vector with one entry per particle")

    def __call__(self, *args):
        return None

    def __repr__(self):
        return "DroguedParticleDynamics{Vector{Float64}}"


def _symbols(names):
    """a tuple of Symbols as Julia shows it: (), (:x,), (:x, :y, :z)"""
    names = list(names)
    if not names:
        return "()"
    if len(names) == 1:
        return f"(:{names[0]},)"
    return "(" + ", ".join(f":{n}" for n in names) + ")"


class LagrangianParticles:
    """LagrangianParticles(; x, y, z, restitution = 1.0, dynamics = no_dynamics, parameters = nothing) and the StructArray constructor's
    tracked_fields and custom properties (LagrangianParticleTracking.jl:60-102): every further keyword is a property, an array with one
    entry per particle; tracked_fields maps a property to the NAME of a model field ("u", "T", "p", "pHY", "νₑ") whose value at the
    particle the property holds after every step.

    Given to NonhydrostaticModel(particles = ...), the model keeps its own bound copy: model.particles.x (.y, .z, .<property>) are numpy
    copies of the current values, model.particles.set(x = ...) writes them."""

    def __init__(self, x, y, z, restitution=1.0, dynamics=None, parameters=None, tracked_fields=None, **properties):
        x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
        if not (x.shape == y.shape == z.shape):
            raise ValueError("x, y, z must all have the same size!")
        if not (x.ndim == 1 and y.ndim == 1 and z.ndim == 1):
            raise ValueError(f"x, y, z must have dimension 1 but ndims=({x.ndim}, {y.ndim}, {z.ndim})")
        self._values = {"x": x.copy(), "y": y.copy(), "z": z.copy()}
        for name, a in properties.items():
            a = np.asarray(a, dtype=np.float64)
            if a.shape != x.shape:
                raise ValueError(f"property {name} must have one entry per particle: shape {a.shape} != {x.shape}")
            self._values[name] = a.copy()
        self.restitution = float(restitution)
        self.tracked_fields = dict(tracked_fields or {})
        for name, field in self.tracked_fields.items():
            if name not in self._values:
                raise ValueError(f"{name} is a tracked field but {self.eltype} has no {name} field! "
                                 "You might have to define your own particle type.")
            if not isinstance(field, str):
                raise NotImplementedError(f"tracked field {name}: only the name of a model field is served; computed fields "
                                          "(AbstractOperations such as √(u² + v²)) are outside the accelerated path")
        if len(self.tracked_fields) > MAX_TRACKED:
            raise NotImplementedError(f"at most {MAX_TRACKED} tracked fields")
        if dynamics is None:
            dynamics = no_dynamics
        if isinstance(dynamics, DroguedParticleDynamics):
            if dynamics.depths.shape != x.shape:
                raise ValueError(f"DroguedParticleDynamics: depths must have one entry per particle ({dynamics.depths.shape} != {x.shape})")
        elif dynamics is not no_dynamics:
            raise NotImplementedError("dynamics must be no_dynamics or DroguedParticleDynamics(depths): a callable cannot cross the C ABI")
        self.dynamics, self.parameters = dynamics, parameters
        self._model = None

    # ---- LagrangianParticleTracking.jl:104-123 ----------------------------------------------------------------------
    @property
    def property_names(self):
        return tuple(self._values)

    @property
    def eltype(self):
        return "Particle" if tuple(self._values) == ("x", "y", "z") else "CustomParticle"

    def __len__(self):
        return int(self._values["x"].shape[0])

    @property
    def size(self):
        return (len(self),)

    def summary(self):
        return f"{len(self)} LagrangianParticles with eltype {self.eltype} and properties {_symbols(self._values)}"

    def __repr__(self):
        dynamics = "no_dynamics" if self.dynamics is no_dynamics else repr(self.dynamics)
        return (f"{len(self)} LagrangianParticles with eltype {self.eltype}:\n"
                f"├── {len(self._values)} properties: {_symbols(self._values)}\n"
                f"├── particle-wall restitution coefficient: {self.restitution!r}\n"
                f"├── {len(self.tracked_fields)} tracked fields: {_symbols(self.tracked_fields)}\n"
                f"└── dynamics: {dynamics}")

    # ---- values: the host arrays, or the model's device arrays once bound ---------------------------------------------
    def _on_device(self, name):
        return self._model is not None and (name in ("x", "y", "z") or name in self.tracked_fields)

    def __getattr__(self, name):
        values = self.__dict__.get("_values")
        if values is None or name not in values:
            raise AttributeError(name)
        if self._on_device(name):
            model = self._model()
            if model is None or model.handle is None:
                raise _lib.OcnError("the model of these particles has been destroyed")
            out = np.empty(len(self), dtype=np.float64)
            buf = out if len(self) else np.empty(1)
            _lib.check(_lib.lib().ocn_model_particle_property(model.handle, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_double))))
            return out
        return values[name].copy()

    def set(self, **values):
        """particles.properties.<name> .= values"""
        for name, a in values.items():
            if name not in self._values:
                raise ValueError(f"the particles have no property {name}")
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), self._values["x"].shape))
            self._values[name] = a.copy()
            if self._on_device(name):
                model = self._model()
                buf = self._values[name] if len(self) else np.empty(1)
                _lib.check(_lib.lib().ocn_model_set_particle_property(model.handle, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_double))))
        return self

    def _bind(self, model, field_names):
        """the model's own copy, its particles uploaded; field_names: property -> the library's name of the tracked field"""
        bound = copy.copy(self)
        bound._values = {n: a.copy() for n, a in self._values.items()}
        bound.tracked_fields = dict(self.tracked_fields)
        n = len(bound)
        dp = C.POINTER(C.c_double)
        pad = lambda a: (a if n else np.zeros(1)).ctypes.data_as(dp)                       # noqa: E731   (n = 0: arrays, not NULL)
        depths = pad(bound.dynamics.depths) if isinstance(bound.dynamics, DroguedParticleDynamics) else None
        L = _lib.lib()
        _lib.check(L.ocn_model_set_particles(model.handle, n, pad(bound._values["x"]), pad(bound._values["y"]), pad(bound._values["z"]),
                                             bound.restitution, depths))
        bound._model = weakref.ref(model)
        for name, cname in field_names.items():
            _lib.check(L.ocn_model_track_particle_field(model.handle, name.encode(), cname.encode()))
            _lib.check(L.ocn_model_set_particle_property(model.handle, name.encode(), pad(bound._values[name])))
        return bound


def validate_particles(particles, grid, tracer_names, has_buoyancy, has_eddy_viscosity):
    """what the model constructor checks before any handle exists -> {property: the library's name of its tracked field}"""
    if particles is None:
        return {}
    if not isinstance(particles, LagrangianParticles):
        raise TypeError("particles must be nothing or LagrangianParticles(...)")
    if hasattr(grid, "local"):
        raise NotImplementedError("particles are not served on partitioned grids (they would have to migrate between ranks)")
    import unicodedata
    names = {}
    for prop, field in particles.tracked_fields.items():
        key = unicodedata.normalize("NFKC", field)
        if key in ("u", "v", "w"):
            names[prop] = key
        elif field in tracer_names:
            names[prop] = "c%d" % tuple(tracer_names).index(field)
        elif key in ("p", "pNHS"):
            names[prop] = "p"
        elif key == "pHY" and has_buoyancy:
            names[prop] = "pHY"
        elif key in ("νe", "nu_e") and has_eddy_viscosity:
            names[prop] = "nu_e"
        else:
            raise ValueError(f"tracked field {prop}: the model has no field {field}")
    return names
