"""numpy restatement of getbc(::ContinuousBoundaryFunction) (BoundaryConditions/continuous_boundary_function.jl:104-154,
Utils/user_function_arguments.jl:22-39): the user's function itself, called on numpy arrays -- the boundary's tangential node coordinates
(Flat ones dropped), a scalar t, the dependencies at the boundary-normal index 1 / N interpolated on their haloed parents to the
condition's location (no interpolation along the normal, none along a Flat direction; two directions nest with the lower one innermost,
Operators/interpolation_operators.jl:45-71) and the parameters when there are some. Also a small interpreter of ocn_expr_ins_t programs.

Sides are 0..5 = west, east, south, north, bottom, top; locations are 3-tuples of the product's Center / Face classes; arrays come back
with shape (Na, Nb): the interior extents of the two tangential directions, x before y before z."""
import numpy as np

SIDES = ("west", "east", "south", "north", "bottom", "top")


def _tangential(side):
    d = side // 2
    return (1, 2) if d == 0 else ((0, 2) if d == 1 else (0, 1))


def _is_face(l):
    return l is not None and l.__name__ == "Face"


def _is_flat(grid, q):
    return grid.topology[q].__name__ == "Flat"


def boundary_coordinates(grid, loc, side):
    """X of x_boundary_node .. z_boundary_node: the two tangential coordinates as (Na, 1) and (1, Nb) arrays, Flat directions dropped;
    and all = the same per tangential direction (None where dropped)"""
    ta, tb = _tangential(side)
    from oldoceananigans_jl_amd import Center
    nodes = grid.nodes(tuple(l if l is not None else Center for l in loc))       # (the tangential nodes do not depend on the normal entry)
    out, both = [], []
    for axis, q in enumerate((ta, tb)):
        if _is_flat(grid, q):
            both.append(None)
            continue
        x = np.asarray(nodes[q]).reshape(-1)[:grid.size[q]]
        x = x.reshape((-1, 1) if axis == 0 else (1, -1))
        out.append(x)
        both.append(x)
    return out, both


def dependency_at_boundary(grid, parent, dep_loc, loc, side):
    """▶(dependency)[i, j, k] with the boundary-normal index 1 (left) or N (right): an (Na, Nb) array"""
    d, right = side // 2, side & 1
    ta, tb = _tangential(side)
    N, H = grid.size, grid.halo_size
    index = [slice(None)] * 3
    index[d] = H[d] + (N[d] - 1 if right else 0)
    slab = np.asarray(parent)[tuple(index)]                     # axes: ta, tb (parent indices, halos included)

    def along(a, axis, q):
        """points 1..N[q] of direction q along `axis`, interpolated from dep_loc[q] to loc[q]"""
        def take(first):                                        # 1-based indices first .. first + N - 1
            sl = [slice(None)] * a.ndim
            sl[axis] = slice(first - 1 + H[q], first - 1 + H[q] + N[q])
            return a[tuple(sl)]
        if _is_flat(grid, q) or _is_face(dep_loc[q]) == _is_face(loc[q]):
            return take(1)
        if _is_face(loc[q]):
            return 0.5 * (take(0) + take(1))                    # ℑᶠ: f[i - 1], f[i]
        return 0.5 * (take(1) + take(2))                        # ℑᶜ: f[i], f[i + 1]

    return along(along(slab, 0, ta), 1, tb)                     # the lower direction innermost


def evaluate(func, grid, loc, side, deps, t, parameters=None):
    """func(X..., t, deps..., [parameters]) on numpy arrays; deps: (parent array, location) pairs"""
    X, _ = boundary_coordinates(grid, loc, side)
    ta, tb = _tangential(side)
    values = [dependency_at_boundary(grid, parent, dep_loc, loc, side) for parent, dep_loc in deps]
    args = X + [float(t)] + values + ([parameters] if parameters is not None else [])
    out = np.empty((grid.size[ta], grid.size[tb]), dtype=np.float64, order="F")
    out[...] = func(*args)
    return out


def interpret(program, coordinates, t, dependencies, shape):
    """the program (a list of (op, a, b, c, imm), OCN_EXPR_* codes) on numpy arrays: coordinates[0 / 1] along the first / second tangential
    direction, dependencies[slot] as (Na, Nb) arrays"""
    binary = {4: np.add, 5: np.subtract, 6: np.multiply, 7: np.divide, 10: np.minimum, 11: np.maximum, 18: np.power, 19: np.less,
              20: np.less_equal, 21: np.greater, 22: np.greater_equal}
    unary = {8: np.negative, 9: np.abs, 12: np.sqrt, 13: np.exp, 14: np.log, 15: np.sin, 16: np.cos, 17: np.tanh}
    v = []
    with np.errstate(all="ignore"):
        for op, a, b, c, imm in program:
            if op == 0: r = np.full(shape, imm)
            elif op == 1: r = np.broadcast_to(coordinates[a], shape)
            elif op == 2: r = np.full(shape, float(t))
            elif op == 3: r = dependencies[a]
            elif op in binary: r = binary[op](v[a], v[b]).astype(np.float64)
            elif op in unary: r = unary[op](v[a])
            elif op == 23: r = np.where(v[a] != 0, v[b], v[c])
            else: raise ValueError(f"unknown op {op}")
            v.append(np.asarray(r, dtype=np.float64))
    return np.asfortranarray(np.broadcast_to(v[-1], shape))
