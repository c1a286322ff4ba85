"""Two independent routes to what a stencil program computes (oldoceananigans_jl_amd/operators.py, include/ocn_mi355x.h), on haloed host
parents:

(a) interpret(): a numpy interpreter of recorded programs, instruction by instruction -- the twin of boundary_functions.interpret. One
    numpy operation per instruction; numpy's + - * / sqrt are the IEEE operations, so with contraction off on the device the bits agree.
(b) the named diagnostics written directly with numpy slices, never through the recorder: ∂z(T), w ∂z(T) at ccf and at ccc, ζ₃ᶠᶠᶜ,
    (u² + v² + w²) / 2 at ccc, divᶜᶜᶜ, znode; ΣᵢⱼΣᵢⱼᶜᶜᶜ is tests/smagorinsky_reference.strain_squared.

plan_slots() restates ocn_stencil_plan's linear scan. KERNEL_FUNCTIONS holds the kernel functions of the named diagnostics, written with
ocn.operators as a user would write them."""
import numpy as np

import smagorinsky_reference as SR
from oldoceananigans_jl_amd import operators as O
from oldoceananigans_jl_amd.grids import Center, Face, Flat

CCC, FCC, CFC, CCF, FFC = (Center,) * 3, (Face, Center, Center), (Center, Face, Center), (Center, Center, Face), (Face, Face, Center)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the interpreter
# ---------------------------------------------------------------------------------------------------------------------
def _window(grid, a, nout, off):
    """the haloed array a over the nout output points, shifted by off"""
    H = grid.halo_size
    return a[tuple(slice(H[d] + off[d], H[d] + off[d] + nout[d]) for d in range(3))]


def _line(table, d, start, n):
    shape = [1, 1, 1]
    shape[d] = n
    return np.asarray(table[start:start + n], dtype=np.float64).reshape(shape)


def interpret(program, grid, location, parents):
    """the interior of the operation at `location`; parents[slot]: the haloed host array of argument `slot`"""
    nout, H = grid.interior_size(location), grid.halo_size
    nodes = ((grid.xᶠᵃᵃ, grid.xᶜᵃᵃ), (grid.yᵃᶠᵃ, grid.yᵃᶜᵃ), (grid.zᵃᵃᶠ, grid.zᵃᵃᶜ))
    unary = {"neg": np.negative, "abs": np.abs, "sqrt": np.sqrt, "exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "tanh": np.tanh}
    binary = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "min": np.minimum, "max": np.maximum, "pow": np.power}
    compare = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}
    with np.errstate(all="ignore"):
        v = []
        for op, a, b, c, di, dj, dk, imm in program:
            k, off = O.OP_NAMES[op], (di, dj, dk)
            if k == "const":
                r = np.float64(imm)
            elif k == "load":
                r = _window(grid, parents[a], nout, off)
            elif k == "spacing":
                if grid.topology[a] is Flat:
                    r = np.float64(1.0)
                elif a < 2:
                    r = np.float64(grid.Δxᶜᵃᵃ if a == 0 else grid.Δyᵃᶜᵃ)
                else:
                    r = _line(grid.Δzᵃᵃᶠ if b == 1 else grid.Δzᵃᵃᶜ, 2, H[2] + dk, nout[2])
            elif k == "node":
                table = nodes[a][0 if b == 1 else 1]
                r = _line(table, a, (0 if grid.topology[a] is Flat else H[a]) + off[a], nout[a])
            elif k in compare:
                r = compare[k](v[a], v[b]).astype(np.float64)
            elif k == "select":
                r = np.where(v[a] != 0.0, v[b], v[c])
            elif k in binary:
                r = binary[k](v[a], v[b])
            else:
                r = unary[k](v[a])
            v.append(r)
        return np.array(np.broadcast_to(v[-1], nout), dtype=np.float64)


def plan_slots(program):
    """ocn_stencil_plan restated: at instruction q the slots of the operands nobody uses later are freed first, q takes the lowest free
    slot, a value nobody uses frees its slot at once, the last value stays. Returns (slot of every value, number of slots)."""
    n = len(program)
    operands = [ins[1:1 + O.ARITY[O.OP_NAMES[ins[0]]]] for ins in program]
    last = list(range(n))
    for q, ops in enumerate(operands):
        for x in ops:
            last[x] = q
    last[n - 1] = n
    used, slot = set(), [0] * n
    for q, ops in enumerate(operands):
        for x in ops:
            if last[x] == q:
                used.discard(slot[x])
        s = 0
        while s in used:
            s += 1
        slot[q] = s
        used.add(s)
        if last[q] == q:
            used.discard(s)
    return slot, max(slot) + 1


def assert_no_shared_live_slot(program, slot):
    """no two values that are alive at the same time share a slot: value x is alive from its definition until its last use (read before
    the user's own result is written, so the user may take x's slot)"""
    n = len(program)
    last = list(range(n))
    for q, ins in enumerate(program):
        for x in ins[1:1 + O.ARITY[O.OP_NAMES[ins[0]]]]:
            last[x] = q
    last[n - 1] = n
    for x in range(n):
        for y in range(x + 1, n):
            if slot[x] == slot[y]:
                assert last[x] <= y, (x, y, slot[x], last[x])


# ---------------------------------------------------------------------------------------------------------------------
# kernel functions of the named diagnostics, as a user writes them
# ---------------------------------------------------------------------------------------------------------------------
def dzT_kernel(i, j, k, grid, T):
    return O.dzᶜᶜᶠ(i, j, k, grid, T)


def w_dzT_ccf_kernel(i, j, k, grid, w, T):
    return w[i, j, k] * O.dzᶜᶜᶠ(i, j, k, grid, T)


def ϕ2(i, j, k, grid, ϕ):
    return ϕ[i, j, k] ** 2


def kinetic_energy_kernel(i, j, k, grid, u, v, w):
    return (O.ℑxᶜᵃᵃ(i, j, k, grid, ϕ2, u) + O.ℑyᵃᶜᵃ(i, j, k, grid, ϕ2, v) + O.ℑzᵃᵃᶜ(i, j, k, grid, ϕ2, w)) / 2


def znode_kernel(i, j, k, grid):
    return O.znode(i, j, k, grid, Center(), Center(), Center())


# ΣᵢⱼΣᵢⱼᶜᶜᶜ as TurbulenceClosures/velocity_tracer_gradients.jl:25-46,78 and Smagorinskys/scale_invariant_operators.jl:10-13 write it
def Σ11(i, j, k, grid, u, v, w): return O.dxᶜᶜᶜ(i, j, k, grid, u)
def Σ22(i, j, k, grid, u, v, w): return O.dyᶜᶜᶜ(i, j, k, grid, v)
def Σ33(i, j, k, grid, u, v, w): return O.dzᶜᶜᶜ(i, j, k, grid, w)
def Σ12(i, j, k, grid, u, v, w): return 0.5 * (O.dyᶠᶠᶜ(i, j, k, grid, u) + O.dxᶠᶠᶜ(i, j, k, grid, v))
def Σ13(i, j, k, grid, u, v, w): return 0.5 * (O.dzᶠᶜᶠ(i, j, k, grid, u) + O.dxᶠᶜᶠ(i, j, k, grid, w))
def Σ23(i, j, k, grid, u, v, w): return 0.5 * (O.dzᶜᶠᶠ(i, j, k, grid, v) + O.dyᶜᶠᶠ(i, j, k, grid, w))
def Σ12sq(*a): return Σ12(*a) ** 2
def Σ13sq(*a): return Σ13(*a) ** 2
def Σ23sq(*a): return Σ23(*a) ** 2
def tr_Σsq(*a): return Σ11(*a) ** 2 + Σ22(*a) ** 2 + Σ33(*a) ** 2


def ΣᵢⱼΣᵢⱼᶜᶜᶜ(i, j, k, grid, u, v, w):
    return (tr_Σsq(i, j, k, grid, u, v, w) + 2 * O.ℑxyᶜᶜᵃ(i, j, k, grid, Σ12sq, u, v, w) + 2 * O.ℑxzᶜᵃᶜ(i, j, k, grid, Σ13sq, u, v, w)
            + 2 * O.ℑyzᵃᶜᶜ(i, j, k, grid, Σ23sq, u, v, w))


# name -> (location, kernel function, names of the field arguments)
KERNEL_FUNCTIONS = {
    "dzT": (CCF, dzT_kernel, "T"),
    "w_dzT_ccf": (CCF, w_dzT_ccf_kernel, "wT"),
    "w_dzT_ccc": (CCC, lambda i, j, k, grid, w, T: O.ℑzᵃᵃᶜ(i, j, k, grid, w) * O.ℑzᵃᵃᶜ(i, j, k, grid, O.dzᶜᶜᶠ, T), "wT"),
    "vorticity": (FFC, O.ζ3ᶠᶠᶜ, "uv"),
    "kinetic_energy": (CCC, kinetic_energy_kernel, "uvw"),
    "divergence": (CCC, O.divᶜᶜᶜ, "uvw"),
    "znode": (CCC, znode_kernel, ""),
    "strain": (CCC, ΣᵢⱼΣᵢⱼᶜᶜᶜ, "uvw"),
}


# ---------------------------------------------------------------------------------------------------------------------
# (b) the same with numpy slices
# ---------------------------------------------------------------------------------------------------------------------
class Slices:
    """windows of haloed parents over the interior of `location`, and the grid's metrics there; Flat directions as the reference's Flat
    methods: a difference is 0, an interpolation the identity, a spacing 1"""

    def __init__(self, grid, location):
        self.grid, self.nout, self.flat = grid, grid.interior_size(location), [t is Flat for t in grid.topology]
        self.dx = 1.0 if self.flat[0] else float(grid.Δxᶜᵃᵃ)
        self.dy = 1.0 if self.flat[1] else float(grid.Δyᵃᶜᵃ)

    def __call__(self, a, di=0, dj=0, dk=0):
        return _window(self.grid, a, self.nout, (di, dj, dk))

    def dz(self, face, dk=0):
        if self.flat[2]:
            return 1.0
        return _line(self.grid.Δzᵃᵃᶠ if face else self.grid.Δzᵃᵃᶜ, 2, self.grid.Hz + dk, self.nout[2])

    def δ(self, d, f, hi, lo):
        """f(hi) - f(lo) along d, 0 when d is Flat; f(shift) -> array"""
        return 0.0 if self.flat[d] else f(hi) - f(lo)

    def ℑ(self, d, f, lo, hi):
        return f(0) if self.flat[d] else 0.5 * (f(lo) + f(hi))


def _full(x, nout):
    return np.array(np.broadcast_to(x, nout), dtype=np.float64)


def dzT(grid, T):
    S = Slices(grid, CCF)
    return _full(S.δ(2, lambda s: S(T, 0, 0, s), 0, -1) * (1 / S.dz(True)), S.nout)


def w_dzT_ccf(grid, w, T):
    S = Slices(grid, CCF)
    return _full(S(w) * (S.δ(2, lambda s: S(T, 0, 0, s), 0, -1) * (1 / S.dz(True))), S.nout)


def w_dzT_ccc(grid, w, T):
    S = Slices(grid, CCC)
    d = lambda s: S.δ(2, lambda t: S(T, 0, 0, s + t), 0, -1) * (1 / S.dz(True, s))          # noqa: E731   ∂z(T) at face k + s
    return _full(S.ℑ(2, lambda s: S(w, 0, 0, s), 0, 1) * S.ℑ(2, d, 0, 1), S.nout)


def vorticity(grid, u, v):
    S = Slices(grid, FFC)
    Γ = S.δ(0, lambda s: S.dy * S(v, s, 0, 0), 0, -1) - S.δ(1, lambda s: S.dx * S(u, 0, s, 0), 0, -1)
    return _full(Γ * (1 / (S.dx * S.dy)), S.nout)


def kinetic_energy(grid, u, v, w):
    S = Slices(grid, CCC)
    sq = lambda a: a * a                                                                   # noqa: E731
    s = S.ℑ(0, lambda s: sq(S(u, s, 0, 0)), 0, 1) + S.ℑ(1, lambda s: sq(S(v, 0, s, 0)), 0, 1)
    return _full((s + S.ℑ(2, lambda s: sq(S(w, 0, 0, s)), 0, 1)) / 2, S.nout)


def divergence(grid, u, v, w):
    S = Slices(grid, CCC)
    dz = S.dz(False)
    Ax, Ay, Az = S.dy * dz, S.dx * dz, S.dx * S.dy
    s = S.δ(0, lambda s: Ax * S(u, s, 0, 0), 1, 0) + S.δ(1, lambda s: Ay * S(v, 0, s, 0), 1, 0)
    return _full((1 / (Az * dz)) * (s + S.δ(2, lambda s: Az * S(w, 0, 0, s), 1, 0)), S.nout)


def znode(grid):
    n = grid.interior_size(CCC)
    return _full(_line(grid.zᵃᵃᶜ, 2, 0 if grid.topology[2] is Flat else grid.Hz, n[2]), n)


def strain(grid, u, v, w):
    m = SR.Metrics(grid)
    return np.array(SR.strain_squared(m, u, v, w, m.interior()), dtype=np.float64)


SLICES = {"dzT": dzT, "w_dzT_ccf": w_dzT_ccf, "w_dzT_ccc": w_dzT_ccc, "vorticity": vorticity, "kinetic_energy": kinetic_energy,
          "divergence": divergence, "znode": znode, "strain": strain}
