"""States outside the O(1) binades the rest of the suite lives in, shared by the host test (the oracle alone certifies that every state
is a fair question) and the GPU test (the tendency kernels against the oracle, bit for bit): powers-of-two ladders of noise and of
plateau-and-step fields, one non-finite cell on a tile seam or a wall, a patch of fluid exactly at rest.

Ladders are powers of two because scaling by 2^k is exact: every rung holds the same significands, so a rung that differs from its
neighbours differs through an exponent range alone (the Float32 reciprocal inside newton_div, the Float64 weight normalisation)."""
import zlib
from collections import namedtuple

import numpy as np

from helpers import ORACLE_TOPO, tanh_faces

P, B = "Periodic", "Bounded"
GridCase = namedtuple("GridCase", "name size topology stretched ntracers impls")

GRIDS = {
    # two 64-wide x tiles with a ragged tail, two row tiles of 7: the all-fields and the role kernel serve it besides the per-field ones
    "A": GridCase("A", (70, 9, 8), (P, P, B), True, 2, (0, 1, 2)),
    # walls everywhere: the per-field kernels with their WENO{2} / UpwindBiased{1} fall-backs (every tendency_impl lands there)
    "B": GridCase("B", (12, 10, 8), (B, B, B), False, 2, (0, 1, 2)),
}

FIELDS = ("u", "v", "w", "c0", "c1")
GPU_NAMES = ("u", "v", "w", "T", "S")
FACE_DIRECTION = {"u": 0, "v": 1, "w": 2}

NOISE_RUNGS = (-600, -300, -60, -27, 0, 20, 31, 40, 55, 58, 60, 61, 62, 63, 64, 66, 100, 300, 500)
PLATEAU_RUNGS = (0, 20, 30, 40, 60, 63, 70, 200)
LADDER = [("noise", k) for k in NOISE_RUNGS] + [("plateau", k) for k in PLATEAU_RUNGS]

# The kernels' Float32 reciprocal is the reference's only while its argument beta + eps stays below 2^126 (ocn_device.h). IN_DOMAIN: the
# rungs on which EVERY smoothness indicator of every field does (test_value_domain_host.py checks this split with largest_indicator):
# there the kernels owe the oracle's bits. On the others they are known to differ, and the GPU test pins what was measured.
FLOAT32_RECIPROCAL_LIMIT = 2.0 ** 126
IN_DOMAIN = [("noise", k) for k in NOISE_RUNGS if k <= 58] + [("plateau", k) for k in PLATEAU_RUNGS if k <= 60]
OUT_OF_DOMAIN = [c for c in LADDER if c not in IN_DOMAIN]
# (grid, state, rung) -> (cells whose bits differ from the oracle's, non-finite cells), summed over the five tendencies' parent arrays;
# the same for every tendency_impl. Measured on the MI355X; the oracle is finite on all of them.
OBSERVED_DEVIATION = {
    ("A", "noise", 60): (18276, 1619), ("A", "noise", 61): (24288, 18276), ("A", "noise", 62): (24568, 24288),
    ("A", "noise", 63): (24570, 24568), ("A", "noise", 64): (24570, 24570), ("A", "noise", 66): (24570, 24570),
    ("A", "noise", 100): (24570, 24570), ("A", "noise", 300): (24570, 24570), ("A", "noise", 500): (24570, 24570),
    ("A", "plateau", 63): (20853, 20853), ("A", "plateau", 70): (21133, 21133), ("A", "plateau", 200): (21133, 21133),
    ("B", "noise", 60): (2604, 174), ("B", "noise", 61): (4036, 2604), ("B", "noise", 62): (4330, 4036),
    ("B", "noise", 63): (4448, 4330), ("B", "noise", 64): (4476, 4448), ("B", "noise", 66): (4486, 4484),
    ("B", "noise", 100): (4488, 4488), ("B", "noise", 300): (4488, 4488), ("B", "noise", 500): (4488, 4488),
    ("B", "plateau", 63): (3384, 3384), ("B", "plateau", 70): (3762, 3762), ("B", "plateau", 200): (3762, 3762),
}

# 0-based interior cells. Grid A: the 64 | 65 tile seam in x and the 7 | 8 row seam in y, the last cell before either seam, the periodic
# wrap in x and y, the last cell of x, y and z. Grid B: one cell beside a wall per field (west, north, bottom, east and top).
NONFINITE_CELLS = {
    "A": (("u", (64, 7, 3)), ("c0", (63, 6, 4)), ("w", (0, 0, 4)), ("v", (69, 8, 7))),
    "B": (("u", (1, 4, 3)), ("v", (5, 9, 2)), ("w", (3, 2, 1)), ("c0", (11, 5, 7))),
}
# fields a non-finite value in `field` reaches: a velocity advects everything, a tracer only itself
REACH = {"u": FIELDS, "v": FIELDS, "w": FIELDS, "c0": ("c0",), "c1": ("c1",)}

# Which side an upwind reconstruction SELECTS, made visible: a product with an advecting velocity of 0, or a sum weighted with 0 and 1,
# hides the unselected side of a finite field, but 0 * NaN is NaN. Each case is noise(0) with one NaN in c0 at `cell`, the velocities of
# `pins` set to exact values, and a cell `clean` whose Gc0 the reference keeps finite only because it selects:
#   tie:  u = 0.0 at the x face f between cells f-1 and f, the NaN at cell f-3 -- in the left-biased WENO{3} stencil (f-3 .. f+1) and not in
#         the right-biased one (f-2 .. f+2). `ut > 0` is false, the right-biased side is taken, Gc0 at cell f stays finite (its other
#         face f+1 reaches down to f-2 only); a kernel that takes the left side at the tie writes NaN there.
#   wall: the two faces of the cell beside a wall are UpwindBiased{1}. With u > 0 at the face between cells 0 and 1 the left cell 0 is
#         taken and a NaN in cell 1 stays out of Gc0 at cell 0; with u < 0 at the face between the last two cells, the mirror image.
#         A kernel that forms left * s2 + (1 - left) * s3 writes NaN there.
# (name, cell of the NaN in c0, {(velocity, index): value}, clean cell); 0-based interior indices
SELECTION_CASES = {
    "A": (("tie-at-the-tile-seam", (61, 6, 4), {("u", (64, 6, 4)): 0.0}, (64, 6, 4)),
          ("tie-at-the-wrap", (67, 2, 5), {("u", (0, 2, 5)): 0.0}, (0, 2, 5))),
    "B": (("tie", (3, 4, 3), {("u", (6, 4, 3)): 0.0}, (6, 4, 3)),
          ("west-wall", (1, 4, 3), {("u", (1, 4, 3)): 0.75}, (0, 4, 3)),
          ("east-wall", (10, 5, 2), {("u", (11, 5, 2)): -0.75}, (11, 5, 2))),
}

# i, j, k slices of the 10 x 4 x 3 block at rest: across both seams of grid A, in the interior of grid B
REST_BLOCK = {"A": (slice(58, 68), slice(4, 8), slice(2, 5)), "B": (slice(1, 11), slice(3, 7), slice(2, 5))}


def z_of(grid):
    if grid.stretched:
        return tanh_faces(grid.size[2])
    return (-1.0, 0.0) if grid.topology[2] == B else (0.0, 1.0)


def oracle_grid(oracle, grid):
    return oracle.Grid(grid.size, topology=tuple(ORACLE_TOPO[t] for t in grid.topology), x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(grid))


def interior_shape(grid, name):
    """N cells, N + 1 faces along a Bounded direction"""
    d = FACE_DIRECTION.get(name)
    return tuple(n + (1 if q == d and grid.topology[q] == B else 0) for q, n in enumerate(grid.size))


def _rng(grid, state):
    """one seed per (grid, kind of state): the rungs of a ladder are the SAME numbers at another exponent"""
    return np.random.default_rng(zlib.crc32(f"{grid.name}-{state}".encode()))


def _unit_noise(grid):
    rng = _rng(grid, "noise")
    return {n: rng.standard_normal(interior_shape(grid, n)) for n in FIELDS}


def noise(grid, k):
    return {n: np.ldexp(a, k) for n, a in _unit_noise(grid).items()}


def plateau(grid, k):
    """2^k (b + c): b a 0 / 1 pattern constant over blocks of 5 x 3 x 4 cells, c = -0.5 for the velocities (both signs of the advecting
    velocity) and 0.25 for the tracers. Inside a block the smoothness indicators are exactly 0; beside a step tau is of the order of 4^k."""
    rng = _rng(grid, "plateau")
    out = {}
    for n in FIELDS:
        shape = interior_shape(grid, n)
        blocks = rng.integers(0, 2, size=tuple(-(-s // b) for s, b in zip(shape, (5, 3, 4)))).astype(np.float64)
        b = blocks[np.ix_(np.arange(shape[0]) // 5, np.arange(shape[1]) // 3, np.arange(shape[2]) // 4)]
        out[n] = np.ldexp(b + (-0.5 if n in FACE_DIRECTION else 0.25), k)
    return out


def state_of(grid, state, k):
    return noise(grid, k) if state == "noise" else plateau(grid, k)


def nonfinite_at(grid, field, cell, value=np.nan):
    vals = noise(grid, 0)
    vals[field][cell] = value
    return vals


def selection_state(grid, cell, pins):
    vals = noise(grid, 0)
    vals["c0"][cell] = np.nan
    for (field, index), value in pins.items():
        vals[field][index] = value
    return vals


def rest_patch(grid):
    """noise with u = v = w = 0.0 in a block: every face inside has an advecting velocity of exactly 0, reconstructions of both signs"""
    vals = noise(grid, 0)
    for n in FACE_DIRECTION:
        vals[n][REST_BLOCK[grid.name]] = 0.0
    return vals


class OracleTendencies:
    """one oracle model per grid, reused: set a state, return copies of the five tendencies (parent arrays)"""

    def __init__(self, oracle, grid):
        self.grid = grid
        self.g_cpu = oracle_grid(oracle, grid)
        self.model = oracle.Model(self.g_cpu, grid.ntracers)

    def __call__(self, vals):
        for n in FIELDS:
            self.model.field("G" + n)[...] = 0.0
        self.model.set(enforce_incompressibility=False, **vals)
        self.model.update_state(True)
        return {n: self.model.field("G" + n).copy() for n in FIELDS}

    def parents(self):
        """the five fields of the state set last, halos filled"""
        return [self.model.field(n).copy() for n in FIELDS]


def same_bits(a, b):
    """identical bit patterns on the whole array (so -0.0 != +0.0, inf == inf), NaNs compared by position"""
    na, nb = np.isnan(a), np.isnan(b)
    if a.shape != b.shape or not np.array_equal(na, nb):
        return False
    ua = np.where(na, np.uint64(0), np.ascontiguousarray(a).view(np.uint64))
    ub = np.where(nb, np.uint64(0), np.ascontiguousarray(b).view(np.uint64))
    return bool(np.array_equal(ua, ub))


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements along x, for the host test's conditions on the inputs (magnitudes, not bits: no fused operations)
# ---------------------------------------------------------------------------------------------------------------------
def curvature_indicator_bound_x(c):
    """13/12 (c[i-1] - 2 c[i] + c[i+1])^2: the curvature term every WENO{3} smoothness indicator of the stencil around i contains"""
    d2 = c[:-2] - 2.0 * c[1:-1] + c[2:]
    return 13.0 / 12.0 * d2 * d2


def _beta3(p0, p1, p2, C):
    return p0 * (C[0] * p0 + C[1] * p1 + C[2] * p2) + p1 * (C[3] * p1 + C[4] * p2) + p2 * p2 * C[5]


def newton_div_f32(a, b):
    """newton_div(Float32, a, b) as the oracle evaluates it: an IEEE Float32 reciprocal (0 once Float32(b) overflows), one Newton step"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        inv = (np.float32(1.0) / b.astype(np.float32)).astype(np.float64)
        x = a * inv
        return x + (a - x * b) * inv


def max_weight_sum_x(c, eps=1e-8):
    """the largest sum of the unnormalised weights alpha_r = C_r (1 + (tau / (beta_r + eps))^2) over the left-biased WENO{3} stencils along
    x of the interior array c (stencils that stay inside the array): the argument of the Float64 reciprocal"""
    s = [c[q:c.shape[0] - 5 + q] for q in range(6)]
    b0 = _beta3(s[2], s[3], s[4], (10, -31, 11, 25, -19, 4))
    b1 = _beta3(s[1], s[2], s[3], (4, -13, 5, 13, -13, 4))
    b2 = _beta3(s[0], s[1], s[2], (4, -19, 11, 25, -31, 10))
    tau = np.abs(b0 - b2)
    total = 0.0
    for C, b in ((0.3, b0), (0.6, b1), (0.1, b2)):
        r = newton_div_f32(tau, b + eps)
        total = total + C * (1.0 + r * r)
    return float(np.max(total))


_B3 = ((10, -31, 11, 25, -19, 4), (4, -13, 5, 13, -13, 4), (4, -19, 11, 25, -31, 10))


def largest_indicator(parents):
    """the largest smoothness indicator any reconstruction of these parent arrays (halos filled) can meet: every window of three cells
    along every direction, each WENO{3} coefficient set in both orientations, and the WENO{2} indicator (a squared difference)"""
    top = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for a in parents:
            for d in range(3):
                m = np.moveaxis(a, d, 0)
                if m.shape[0] < 3:
                    continue
                p0, p1, p2 = m[:-2], m[1:-1], m[2:]
                for C in _B3:
                    top = max(top, float(np.max(_beta3(p0, p1, p2, C))), float(np.max(_beta3(p2, p1, p0, C))))
                top = max(top, float(np.max((m[1:] - m[:-1]) ** 2)))
    return top


def largest_weight_sum():
    """max_weight_sum_x over every field of every rung of both ladders on both grids"""
    with np.errstate(over="ignore", invalid="ignore"):
        return max(max_weight_sum_x(a) for grid in GRIDS.values() for state, k in LADDER for a in state_of(grid, state, k).values())
