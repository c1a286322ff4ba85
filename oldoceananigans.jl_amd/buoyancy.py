"""Buoyancy formulations and constant Coriolis terms on the accelerated path (reference: src/BuoyancyFormulations/,
src/Coriolis/): BuoyancyTracer and linear SeawaterBuoyancy, with gravity along -z or, wrapped in a BuoyancyForce, along any unit vector;
FPlane and ConstantCartesianCoriolis."""
from .grids import NegativeZDirection, ZDirection, validate_unit_vector


class BuoyancyTracer:
    """BuoyancyTracer(): the tracer `b` is the buoyancy (buoyancy_tracer.jl:1-12)"""
    required_tracers = ("b",)

    def __repr__(self):
        return "BuoyancyTracer()"


class LinearEquationOfState:
    """LinearEquationOfState(thermal_expansion = 1.67e-4, haline_contraction = 7.80e-4) (linear_equation_of_state.jl:39-41)"""

    def __init__(self, thermal_expansion=1.67e-4, haline_contraction=7.80e-4):
        self.thermal_expansion, self.haline_contraction = float(thermal_expansion), float(haline_contraction)


class SeawaterBuoyancy:
    """SeawaterBuoyancy(equation_of_state = LinearEquationOfState(), gravitational_acceleration = g_Earth): b = g (α T - β S)
    (seawater_buoyancy.jl, linear_equation_of_state.jl:71-73). Nonlinear equations of state (TEOS-10) are third-party code absent
    from the reference tree and stay out of scope."""
    required_tracers = ("T", "S")

    def __init__(self, equation_of_state=None, gravitational_acceleration=9.80665):
        self.equation_of_state = equation_of_state if equation_of_state is not None else LinearEquationOfState()
        if not isinstance(self.equation_of_state, LinearEquationOfState):
            raise NotImplementedError("only LinearEquationOfState is on the accelerated path")
        self.gravitational_acceleration = float(gravitational_acceleration)

    def __repr__(self):
        e = self.equation_of_state
        return (f"SeawaterBuoyancy(g={self.gravitational_acceleration}, LinearEquationOfState(α={e.thermal_expansion}, "
                f"β={e.haline_contraction}))")


def sind(x):
    """sin of an angle in degrees as Julia's `sind` returns it: exact at multiples of 30 and 45 degrees, correctly rounded elsewhere
    (math.sin(math.radians(45)) is one ulp below sind(45) = 0.7071067811865476)"""
    from decimal import Decimal, getcontext
    from fractions import Fraction
    getcontext().prec = 60
    r = Fraction(float(x)) % 360
    sign = 1
    if r >= 180:
        r, sign = r - 180, -1
    if r > 90:
        r = 180 - r
    if r == 0:
        return 0.0 * sign
    if r == 90:
        return 1.0 * sign
    if r == 30:
        return 0.5 * sign
    pi = Decimal("3.14159265358979323846264338327950288419716939937510582097494459")
    t = Decimal(r.numerator) / Decimal(r.denominator) * pi / 180
    term, total, n = t, t, 1
    while abs(term) > Decimal(10) ** -55:
        term = -term * t * t / ((2 * n) * (2 * n + 1))
        total += term
        n += 1
    return float(total) * sign


def cosd(x):
    """cos of an angle in degrees as Julia's `cosd` returns it: sind of the complementary angle, formed exactly"""
    from fractions import Fraction
    return sind(Fraction(90) - Fraction(float(x)))


def _prettysummary(x):
    """prettysummary(::AbstractFloat) (Grids/grid_utils.jl:282): the shortest representation, at most 6 significant digits"""
    return repr(float("%.6g" % x))


class BuoyancyForce:
    """BuoyancyForce(formulation; gravity_unit_vector = NegativeZDirection()) (buoyancy_force.jl:4-50): the buoyancy acceleration acts in
    the direction opposite to gravity; ĝ = -gravity_unit_vector (:52-54)"""

    def __init__(self, formulation, gravity_unit_vector=None):
        if isinstance(formulation, BuoyancyForce):
            raise ValueError("the formulation of a BuoyancyForce is a buoyancy formulation, not another BuoyancyForce")
        self.formulation = formulation
        self.gravity_unit_vector = validate_unit_vector(NegativeZDirection() if gravity_unit_vector is None else gravity_unit_vector)

    @property
    def required_tracers(self):
        return self.formulation.required_tracers

    @property
    def tilted(self):
        """whether gravity is a vector rather than NegativeZDirection()"""
        return not isinstance(self.gravity_unit_vector, NegativeZDirection)

    def summary(self):
        """Base.summary (buoyancy_force.jl:77-85)"""
        g = self.gravity_unit_vector
        vec = "(" + ", ".join(_prettysummary(c) for c in g) + ")" if self.tilted else "NegativeZDirection()"
        return f"{type(self.formulation).__name__} with ĝ = {vec}"

    def __repr__(self):
        return self.summary()


class ConstantCartesianCoriolis:
    """ConstantCartesianCoriolis(fx, fy, fz) | (f, rotation_axis = ZDirection()) | (latitude, rotation_rate): a constant rotation vector
    with all three components (Coriolis/constant_cartesian_coriolis.jl:32-66); the reference's ArgumentErrors are ValueErrors"""

    def __init__(self, fx=None, fy=None, fz=None, f=None, rotation_axis=None, latitude=None, rotation_rate=7.292115e-5):
        rotation_axis = ZDirection() if rotation_axis is None else rotation_axis
        if latitude is not None:
            if not all(c is None for c in (fx, fy, fz, f)):
                raise ValueError("Only `rotation_rate` can be specified when using `latitude`.")
            fx, fy, fz = 0, 2 * rotation_rate * cosd(latitude), 2 * rotation_rate * sind(latitude)
        elif f is not None:
            if not all(c is None for c in (fx, fy, fz, latitude)):
                raise ValueError("Only `rotation_axis` can be specified when using `f`.")
            rotation_axis = validate_unit_vector(rotation_axis)
            if isinstance(rotation_axis, ZDirection):
                fx, fy, fz = 0, 0, f
            elif isinstance(rotation_axis, NegativeZDirection):
                raise ValueError("rotation_axis must be ZDirection() or a unit vector")
            else:
                fx, fy, fz = f * rotation_axis[0], f * rotation_axis[1], f * rotation_axis[2]
        elif all(c is not None for c in (fx, fy, fz)):
            pass                                                 # (latitude and f are nothing here)
        else:
            raise ValueError("Either (i) `latitude`, or (ii) `f`, or (iii) `fx`, `fy` and `fz` must be specified.")
        self.fx, self.fy, self.fz = float(fx), float(fy), float(fz)

    def __repr__(self):
        return "ConstantCartesianCoriolis{Float64}: " + "fx = %.2e, fy = %.2e, fz = %.2e" % (self.fx, self.fy, self.fz)


class FPlane:
    """FPlane(f = ...) | FPlane(rotation_rate = Ω, latitude = φ): f = 2 Ω sind(φ) (Coriolis/f_plane.jl:13-44)"""

    def __init__(self, f=None, rotation_rate=7.292115e-5, latitude=None):
        import math
        if (f is None) == (latitude is None):
            raise ValueError("Either both keywords rotation_rate and latitude must be specified, *or* only f must be specified.")
        self.f = float(f) if f is not None else 2 * rotation_rate * sind(latitude)      # f_plane.jl:38: 2rotation_rate * sind(latitude)

    def __repr__(self):
        return f"FPlane(f={self.f})"
