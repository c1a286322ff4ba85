"""numpy restatement of the diagnostics (csrc/ocn_diagnostics.h) on haloed parent arrays, with the arguments of the library calls
ocn_compute_operation / ocn_reduce_operation / ocn_accumulate_operation: the operand is a mirror of ocn_operand_t whose a / b are HOST parent
arrays. Every value is formed by the reference's operation sequence in IEEE doubles (numpy evaluates elementwise, without fused
multiply-adds), so computed fields, extrema and accumulations compare with `==`; sums are returned with their terms, so a test can bound
them with math.fsum.

reference: Operators/interpolation_operators.jl:8-15,45-71,87-110; AbstractOperations/binary_operations.jl:38-52,109-135;
metric_field_reductions.jl:12-21,65-94,144-150,206-212; Fields/scans.jl:272-306; Fields/field.jl:673-687,722-732"""
import numpy as np

OPS = {0: None, 1: np.add, 2: np.subtract, 3: np.multiply, 4: np.divide}
OP_CODE = {"+": 1, "-": 2, "*": 3, "/": 4}


class Operand:
    """ocn_operand_t with host arrays; locations are tuples of the package's Center / Face classes"""

    def __init__(self, op, a, b, ca, cb, loc_a, loc_b, loc):
        self.op, self.a, self.b, self.ca, self.cb, self.loc_a, self.loc_b, self.loc = op, a, b, ca, cb, loc_a, loc_b, loc


def operand_of(x, parents):
    """the Operand of a package Field or BinaryOperation; parents: {field: host parent array}"""
    if hasattr(x, "interp_a"):
        fa, fb = hasattr(x.a, "loc"), hasattr(x.b, "loc")
        return Operand(OP_CODE[x.op], parents[x.a] if fa else None, parents[x.b] if fb else None, None if fa else float(x.a),
                       None if fb else float(x.b), x.a.loc if fa else None, x.b.loc if fb else None, tuple(x.location))
    return Operand(0, parents[x], None, None, None, x.loc, None, tuple(x.loc))


def _is_face(l):
    return l is not None and l.__name__ == "Face"


def _is_flat(t):
    return t.__name__ == "Flat"


def interpolate(grid, arr, from_loc, to_loc):
    """▶(arr) over the interior of to_loc: 0.5 (f[i] + f[i+1]) to a Center, 0.5 (f[i-1] + f[i]) to a Face, per direction that changes
    location and is not Flat; two directions nest z of y of x, three x of y of z"""
    n, H = grid.interior_size(to_loc), grid.halo_size
    dirs = [d for d in range(3) if from_loc[d] is not to_loc[d] and not _is_flat(grid.topology[d])]
    order = dirs[::-1] if len(dirs) == 3 else dirs                     # innermost first

    def at(off):
        return arr[tuple(slice(H[d] + off[d], H[d] + off[d] + n[d]) for d in range(3))]

    def nest(level, off):
        if level < 0:
            return at(off)
        d = order[level]
        lo = list(off)
        lo[d] += -1 if _is_face(to_loc[d]) else 0
        hi = list(lo)
        hi[d] += 1
        return 0.5 * (nest(level - 1, lo) + nest(level - 1, hi))

    return nest(len(order) - 1, [0, 0, 0])


def metric(grid, loc, dims_mask):
    """reduction_grid_metric(dims) at `loc` over the interior, broadcastable: Δx, Δy, Δz, Az = Δx Δy, Ay = Δx Δz, Ax = Δy Δz, V = Az Δz"""
    x, y, z = dims_mask & 1, dims_mask & 2, dims_mask & 4
    n2 = grid.interior_size(loc)[2]
    dz = (grid.Δzᵃᵃᶠ if _is_face(loc[2]) else grid.Δzᵃᵃᶜ)[grid.Hz:grid.Hz + n2].reshape(1, 1, n2)
    if x or y:
        mc = grid.Δxᶜᵃᵃ * grid.Δyᵃᶜᵃ if (x and y) else (grid.Δxᶜᵃᵃ if x else grid.Δyᵃᶜᵃ)
        return mc * dz if z else np.full((1, 1, 1), mc)
    return dz


def evaluate(grid, operand, dims_mask=0, absolute=False):
    """(operand [abs] [* metric], metric) over the interior of operand.loc; metric is None without one (dims_mask = 0)"""
    a = interpolate(grid, operand.a, operand.loc_a, operand.loc) if operand.a is not None else operand.ca
    v = a
    if operand.op:
        b = interpolate(grid, operand.b, operand.loc_b, operand.loc) if operand.b is not None else operand.cb
        v = OPS[operand.op](a, b)
    v = np.array(v, dtype=np.float64)
    if absolute:
        v = np.abs(v)
    if not dims_mask:
        return v, None
    m = metric(grid, operand.loc, dims_mask)
    return v * m, np.broadcast_to(m, v.shape)


def compute_operation(grid, operand):
    """the interior of the computed field"""
    return evaluate(grid, operand)[0]


def _axes(dims_mask):
    return tuple(d for d in range(3) if dims_mask >> d & 1)


def reduce_terms(grid, operand, dims_mask, use_metric, absolute=False):
    """(terms, metric terms or None, count): what the reduction adds per output element lies along the axes of dims_mask"""
    v, m = evaluate(grid, operand, dims_mask if use_metric else 0, absolute)
    return v, m, int(np.prod([v.shape[d] for d in _axes(dims_mask)]))


def reduce_operation(grid, operand, kind, dims_mask, use_metric, absolute=False):
    """the interior of the reduced field (size 1 along the reduced directions); kind: "sum" | "maximum" | "minimum" | "average". Sums are
    numpy's -- exact for the dyadic test numbers, one admissible order otherwise"""
    v, m, count = reduce_terms(grid, operand, dims_mask, use_metric, absolute)
    ax = _axes(dims_mask)
    if kind == "maximum":
        return np.max(v, axis=ax, keepdims=True)
    if kind == "minimum":
        return np.min(v, axis=ax, keepdims=True)
    s = np.sum(v, axis=ax, keepdims=True)
    if kind == "average":
        return s / (np.sum(m, axis=ax, keepdims=True) if use_metric else count)
    return s


def accumulate_operation(grid, operand, dim, reverse, use_metric):
    """B[start] = A[start], B[i] = B[i ∓ 1] + A[i] along the 0-based direction dim (np.cumsum adds in exactly this order)"""
    v, _ = evaluate(grid, operand, (1 << dim) if use_metric else 0)
    if reverse:
        return np.flip(np.cumsum(np.flip(v, axis=dim), axis=dim), axis=dim)
    return np.cumsum(v, axis=dim)


def evaluate_scan(scan, parents):
    """the interior of Field(scan) for a package scan (Average, Integral, Reduction, CumulativeIntegral, Accumulation)"""
    operand = operand_of(scan.operand, parents)
    if scan.reducing:
        mask = 0
        for d in scan.dims:
            mask |= 1 << (d - 1)
        return reduce_operation(scan.grid, operand, scan.kind, mask, scan.use_metric, scan.absolute)
    return accumulate_operation(scan.grid, operand, scan.dims[0] - 1, scan.reverse, scan.use_metric)
