"""Stokes drift of a surface-wave field (reference: src/StokesDrifts.jl). UniformStokesDrift -- horizontally uniform, the drift of the
Langmuir-turbulence configuration -- is served by the library as six per-level tables (include/ocn_mi355x.h: ocn_model_set_stokes_drift);
StokesDrift, with horizontal structure, exists as a descriptor only and the model refuses it by name.

`∂` is not a letter Python accepts in a keyword written in source, so the reference's keywords are accepted through a dictionary --
UniformStokesDrift(**{"∂z_uˢ": f}) -- and have the ASCII aliases dz_us, dz_vs, dt_us, dt_vs."""
import unicodedata

import numpy as np

from .grids import Flat

_ALIASES = {"∂z_us": "dz_us", "∂z_vs": "dz_vs", "∂t_us": "dt_us", "∂t_vs": "dt_vs"}      # keys after NFKC (ˢ -> s)
_NAMES = (("dz_us", "∂z_uˢ"), ("dz_vs", "∂z_vˢ"), ("dt_us", "∂t_uˢ"), ("dt_vs", "∂t_vˢ"))


def zerofunction(*args):
    """@inline zerofunction(args...) = 0 (StokesDrifts.jl:72)"""
    return 0


def _ascii_keywords(kw, accepted):
    out = {}
    for key, value in kw.items():
        name = _ALIASES.get(unicodedata.normalize("NFKC", key), key)
        if name not in accepted or name in out:
            raise TypeError(f"unexpected or repeated keyword {key!r}")
        out[name] = value
    return out


def _prettysummary(x):
    """prettysummary of a function (its name), a named tuple `(a=1, b=2)`, a number or an array"""
    if callable(x):
        return getattr(x, "__name__", type(x).__name__)
    if isinstance(x, dict) or hasattr(x, "_asdict") or (hasattr(x, "__dict__") and not isinstance(x, np.ndarray)):
        items = x.items() if isinstance(x, dict) else (x._asdict().items() if hasattr(x, "_asdict") else vars(x).items())
        return "(" + ", ".join(f"{k}={_prettysummary(v)}" for k, v in items) + ")"
    if isinstance(x, np.ndarray):
        return f"{x.size}-element Vector{{Float64}}"
    return "nothing" if x is None else repr(x)


class UniformStokesDrift:
    """UniformStokesDrift(; ∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ, parameters = nothing) (StokesDrifts.jl:125-126): functions f(z, t), or f(z, t,
    parameters) when parameters are given; zerofunction by default. UniformStokesDrift(grid; ...) (:128-136): arrays -- ∂z_uˢ, ∂z_vˢ on
    the z faces (Nz + 1 values, the mirror of Field{Nothing, Nothing, Face}), ∂t_uˢ, ∂t_vˢ at the z centres (Nz values), zeros by default.
    Either form also takes a number (a constant) or None (`nothing`: zero) per entry."""

    def __init__(self, grid=None, dz_us=None, dz_vs=None, dt_us=None, dt_vs=None, parameters=None, **reference_keywords):
        given = dict(dz_us=dz_us, dz_vs=dz_vs, dt_us=dt_us, dt_vs=dt_vs)
        for name, value in _ascii_keywords(reference_keywords, given).items():
            if given[name] is not None:
                raise TypeError(f"{name} given twice")
            given[name] = value
        self.grid, self.parameters = grid, parameters
        for name, value in given.items():
            if value is None:
                # the defaults of the two constructors: zerofunction, or a zero Field on the grid (:125, :129-132)
                value = zerofunction if grid is None else np.zeros(grid.Nz + (1 if name.startswith("dz") else 0))
            elif not callable(value) and not np.isscalar(value):
                value = np.array(value, dtype=np.float64)
                if value.ndim != 1:
                    raise ValueError(f"{name}: an array-valued entry is one-dimensional (one value per level), got shape {value.shape}")
            setattr(self, name, value)

    def _table(self, name, z, t):
        """the entry `name` at the nodes z: ∂z_Uᵃᵃᶜ / ∂z_Uᵃᵃᶠ / ∂t_U for a function (StokesDrifts.jl:144-145,151-152,158-159)"""
        f = getattr(self, name)
        if callable(f):
            args = (float(t),) if self.parameters is None else (float(t), self.parameters)
            return np.array([float(f(float(zk), *args)) for zk in z], dtype=np.float64)
        return np.full(len(z), float(f))                # a number

    def tables(self, grid, time=0.0):
        """the six per-level tables of the library at `time`: (dzu_c, dzu_f, dzv_c, dzv_f, dtu_c, dtv_c), with znode(k, grid, Center()) for k
        = 1..Nz and znode(k, grid, Face()) for k = 1..Nz + 1. An array-valued ∂z entry IS the face table and its centre table is ℑzᵃᵃᶜ of it,
        0.5 (a[k] + a[k + 1]) (:146-147,153-154); an array-valued ∂t entry is the centre table (:160-161). ValueError for wrong lengths."""
        Nz, Hz = grid.Nz, grid.Hz
        zc, zf = np.asarray(grid.zᵃᵃᶜ)[Hz:Hz + Nz], np.asarray(grid.zᵃᵃᶠ)[Hz:Hz + Nz + 1]
        out = []
        for name in ("dz_us", "dz_vs"):
            a = getattr(self, name)
            if isinstance(a, np.ndarray):
                if a.shape != (Nz + 1,):
                    raise ValueError(f"{name}: an array on the z faces has Nz + 1 = {Nz + 1} values, got {a.shape[0]}")
                out += [0.5 * (a[:-1] + a[1:]), a.copy()]
            else:
                out += [self._table(name, zc, time), self._table(name, zf, time)]
        for name in ("dt_us", "dt_vs"):
            a = getattr(self, name)
            if isinstance(a, np.ndarray):
                if a.shape != (Nz,):
                    raise ValueError(f"{name}: an array at the z centres has Nz = {Nz} values, got {a.shape[0]}")
                out.append(a.copy())
            else:
                out.append(self._table(name, zc, time))
        return tuple(np.ascontiguousarray(t, dtype=np.float64) for t in out)

    def summary(self):
        """Base.summary (StokesDrifts.jl:55-60)"""
        if self.parameters is None:
            return "UniformStokesDrift{Nothing}"
        return f"UniformStokesDrift with parameters {_prettysummary(self.parameters)}"

    def __repr__(self):
        """Base.show (StokesDrifts.jl:62-68)"""
        marks = ("├── ", "├── ", "├── ", "└── ")
        return self.summary() + ":\n" + "\n".join(f"{m}{shown}: {_prettysummary(getattr(self, name))}" for m, (name, shown) in zip(marks, _NAMES))


class StokesDrift:
    """StokesDrift(; ∂z_uˢ, ∂y_uˢ, ∂t_uˢ, ∂z_vˢ, ∂x_vˢ, ∂t_vˢ, ∂x_wˢ, ∂y_wˢ, ∂t_wˢ, parameters) (StokesDrifts.jl:180-330): a drift with
    horizontal structure. A descriptor only: NonhydrostaticModel refuses it by name."""

    def __init__(self, parameters=None, **terms):
        self.parameters, self.terms = parameters, dict(terms)

    def __repr__(self):
        return "StokesDrift" + ("{Nothing}" if self.parameters is None else f" with parameters {_prettysummary(self.parameters)}")


def validate_stokes_drift(stokes_drift, grid):
    """the refusals that need no table: the kind of drift, a partitioned grid, a Flat z"""
    if stokes_drift is None:
        return
    if isinstance(stokes_drift, StokesDrift):
        raise NotImplementedError("StokesDrift (a Stokes drift with horizontal structure) is not on the accelerated path; "
                                  "stokes_drift must be nothing or a UniformStokesDrift")
    if not isinstance(stokes_drift, UniformStokesDrift):
        raise NotImplementedError("stokes_drift must be nothing or a UniformStokesDrift")
    if hasattr(grid, "local"):
        raise NotImplementedError("a Stokes drift is not served on partitioned grids")
    if grid.topology[2] is Flat:
        raise NotImplementedError("a UniformStokesDrift varies with z: it is not served on a grid whose z direction is Flat")


def regularize_stokes_drift(stokes_drift, grid, time=0.0):
    """what NonhydrostaticModel(stokes_drift = ...) hands to the library: None, or the six tables at the clock's time. Everything is
    settled on the host, before a model handle exists."""
    validate_stokes_drift(stokes_drift, grid)
    if stokes_drift is None:
        return None
    tables = stokes_drift.tables(grid, time)
    # a time step runs all its stages inside the library with ONE set of tables: a drift whose functions change with time would need them
    # refreshed per stage
    later = stokes_drift.tables(grid, time + 1.0)
    if any(not np.array_equal(a, b) for a, b in zip(tables, later)):
        raise NotImplementedError("time dependence of a UniformStokesDrift is not served: its functions must not depend on t")
    return tables
