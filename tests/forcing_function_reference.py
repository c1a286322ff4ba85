"""numpy restatement of a function-valued forcing (Forcings/continuous_forcing.jl:119-142; Relaxation with a function mask or target,
relaxation.jl:80-101): the user's own functions called on numpy arrays -- the node coordinates of the forced field's location (Flat
directions dropped), a scalar t, the dependencies interpolated on their haloed parents to that location (none along a Flat direction; the
lower direction innermost, Operators/interpolation_operators.jl:45-71). Arrays have the interior shape of the location.

Also a restatement of how the library splits a program: the class of every value and the length of the per-cell program."""
import numpy as np

UNIFORM, LINE_X, LINE_Y, LINE_Z, CELL = 0, 1, 2, 3, 4

# value operands per OCN_EXPR_* op (include/ocn_mi355x.h)
ARITY = {0: 0, 1: 0, 2: 0, 3: 0, 8: 1, 9: 1, 12: 1, 13: 1, 14: 1, 15: 1, 16: 1, 17: 1, 23: 3}
ARITY.update({op: 2 for op in (4, 5, 6, 7, 10, 11, 18, 19, 20, 21, 22)})


def _is_face(l):
    return l.__name__ == "Face"


def _is_flat(grid, q):
    return grid.topology[q].__name__ == "Flat"


def coordinates(grid, loc):
    """X: the node coordinates over the interior of `loc`, shaped to broadcast as (x, y, z), Flat directions dropped"""
    n, H = grid.interior_size(loc), grid.halo_size
    nodes = ((grid.xᶠᵃᵃ, grid.xᶜᵃᵃ), (grid.yᵃᶠᵃ, grid.yᵃᶜᵃ), (grid.zᵃᵃᶠ, grid.zᵃᵃᶜ))
    X = []
    for d in range(3):
        if _is_flat(grid, d):
            continue
        shape = [1, 1, 1]
        shape[d] = n[d]
        X.append(np.asarray(nodes[d][0] if _is_face(loc[d]) else nodes[d][1], dtype=np.float64)[H[d]:H[d] + n[d]].reshape(shape))
    return X


def dependency(grid, parent, dep_loc, loc):
    """ℑ(dependency)[i, j, k] over the interior of `loc`, from the haloed parent of a field at dep_loc"""
    n, H = grid.interior_size(loc), grid.halo_size

    def along(a, q):
        def take(first):                                        # 1-based indices first .. first + n - 1
            sl = [slice(None)] * 3
            sl[q] = slice(first - 1 + H[q], first - 1 + H[q] + n[q])
            return a[tuple(sl)]
        if _is_flat(grid, q) or _is_face(dep_loc[q]) == _is_face(loc[q]):
            return take(1)
        if _is_face(loc[q]):
            return 0.5 * (take(0) + take(1))                    # ℑᶠ: f[i - 1], f[i]
        return 0.5 * (take(1) + take(2))                        # ℑᶜ: f[i], f[i + 1]

    return along(along(along(np.asarray(parent), 0), 1), 2)     # the lower direction innermost


def evaluate(func, grid, loc, deps, t):
    """func(X..., t, deps...) on numpy arrays; deps: (parent array, location) pairs"""
    values = [dependency(grid, parent, dep_loc, loc) for parent, dep_loc in deps]
    out = np.empty(grid.interior_size(loc), dtype=np.float64)
    with np.errstate(all="ignore"):
        out[...] = func(*(coordinates(grid, loc) + [float(t)] + values))
    return out


def value_classes(program):
    """per value the set of inputs it depends on out of {x, y, z, field} -- constants and t add nothing -- as a class: uniform (none),
    a line (one coordinate only), cell (two coordinates, or a field)"""
    depends = []
    for op, a, b, c, _ in program:
        s = {("x", "y", "z")[a]} if op == 1 else ({"field"} if op == 3 else set())
        for v in (a, b, c)[:ARITY[op]]:
            s = s | depends[v]
        depends.append(s)
    line = {frozenset("x"): LINE_X, frozenset("y"): LINE_Y, frozenset("z"): LINE_Z}
    return [UNIFORM if not s else line.get(frozenset(s), CELL) for s in depends]


def cell_length(program):
    """the per-cell program: the cell instructions, and one table load per distinct uniform or line value they consume; a result that is
    no cell value is one load"""
    cls = value_classes(program)
    if cls[-1] != CELL:
        return 1
    roots, n = set(), 0
    for q, (op, a, b, c, _) in enumerate(program):
        if cls[q] != CELL:
            continue
        n += 1
        roots |= {v for v in (a, b, c)[:ARITY[op]] if cls[v] != CELL}
    return n + len(roots)
