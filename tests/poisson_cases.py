"""The white-noise cases of the pressure solve, shared by the host test (the oracle against the long-double reference) and the GPU test (the
HIP paths against both): the smallest shapes that reach each size-selected path and each of its edges.

`paths` is what a model on the case's grid must report for ("split_solve_active", "fused_zfft_active", "c2r_strided_active"). The first two
follow from the solver's selection rules (Ny = 2^m in 8 .. 1024 on Periodic x, y with the Fourier-tridiagonal solver or the fused z transform;
FFT solver with Nz = 2^m in 8 .. 1024); the third is rocFFT's answer to the Z2D plan that writes into the haloed field, as it gives it on the MI355X: refused at 128 x 16, 128 x 8, 16 x 16
and 8 x 8 (the solver then keeps the dense plan and a copy), accepted at every other shape here; 0 on complex storage."""
from collections import namedtuple

import numpy as np

import poisson_reference as PR
from helpers import ORACLE_TOPO, tanh_faces

P, B, F = "Periodic", "Bounded", "Flat"

Case = namedtuple("Case", "path topology size stretched kind real_fft paths")


def _c(path, topology, size, kind, paths, stretched=None, real_fft=1):
    return Case(path, topology, size, kind == 1 if stretched is None else stretched, kind, real_fft, paths)


SOLVER_CASES = [
    # split form (1-D x plans on padded rows, strided_line_fft_kernel along y), tridiagonal_z_kernel on the half spectrum
    _c("split-tridiagonal", (P, P, B), (126, 8, 10), 1, (1, 0, 1)),          # Nxh = 64: one full 64-column block
    _c("split-tridiagonal", (P, P, B), (128, 16, 12), 1, (1, 0, 0)),         # Nxh = 65: a one-column second block; Nxp = 72: pitch padding
    _c("split-tridiagonal", (P, P, B), (130, 8, 9), 1, (1, 0, 1)),
    _c("split-tridiagonal", (P, P, B), (10, 64, 12), 1, (1, 0, 1)),
    _c("split-tridiagonal", (P, P, B), (8, 512, 6), 1, (1, 0, 1)),           # line_zl512: 4 lines per workgroup
    _c("split-tridiagonal", (P, P, B), (8, 1024, 6), 1, (1, 0, 1)),
    # 2-D library plans, tridiagonal_z_kernel
    _c("plain-tridiagonal", (P, P, B), (34, 10, 128), 1, (0, 0, 1)),         # deep column
    _c("plain-tridiagonal", (P, P, B), (12, 6, 10), 1, (0, 0, 1)),           # Ny < 8
    _c("plain-tridiagonal", (P, P, B), (9, 7, 3), 1, (0, 0, 1)),             # Nz = Hz
    _c("plain-tridiagonal", (P, P, B), (16, 16, 16), 1, (1, 0, 0), stretched=False),     # regular z: the default solver of a z-Bounded grid
    # FFT solver: split form + fused z transform (zline_solve_kernel)
    _c("split-fused-z", (P, P, P), (126, 8, 8), 0, (1, 1, 1)),
    _c("split-fused-z", (P, P, P), (128, 8, 8), 0, (1, 1, 0)),
    _c("split-fused-z", (P, P, P), (130, 16, 8), 0, (1, 1, 1)),
    _c("split-fused-z", (P, P, P), (8, 8, 256), 0, (1, 1, 0)),
    _c("fused-z", (P, P, P), (12, 10, 32), 0, (0, 1, 1)),                    # 2-D plans + fused z transform
    _c("3d-plans", (P, P, P), (10, 6, 7), 0, (0, 0, 1)),
    # Bounded x / y: gather / scatter cosine transforms on complex storage
    _c("cosine", (P, B, B), (11, 13, 9), 0, (0, 0, 0)),
    _c("cosine", (B, P, B), (11, 13, 9), 0, (0, 0, 0)),
    _c("cosine", (B, B, B), (11, 13, 9), 0, (0, 0, 0)),
    _c("cosine", (P, B, B), (11, 13, 9), 1, (0, 0, 0)),
    _c("cosine", (B, P, B), (11, 13, 9), 1, (0, 0, 0)),
    _c("cosine", (B, B, B), (11, 13, 9), 1, (0, 0, 0)),
    _c("cosine", (B, B, B), (130, 8, 9), 1, (0, 0, 0)),
    # Flat directions are not transformed
    _c("flat", (P, F, B), (66, 1, 16), 1, (0, 0, 0)),
    _c("flat", (B, B, F), (12, 10, 1), 0, (0, 0, 0)),
    # complex-to-complex transforms on a periodic grid (option real_fft = 0)
    _c("complex", (P, P, B), (16, 8, 10), 1, (0, 0, 0), real_fft=0),
]

ModelCase = namedtuple("ModelCase", "topology size stretched ntracers paths")

MODEL_CASES = [
    ModelCase((P, P, P), (16, 8, 8), False, 0, (1, 1, 1)),
    ModelCase((P, P, P), (16, 8, 8), False, 2, (1, 1, 1)),
    ModelCase((P, P, P), (70, 16, 8), False, 2, (1, 1, 1)),                  # a ragged second 64-wide block
    ModelCase((P, P, B), (128, 16, 12), True, 2, (1, 0, 0)),
    ModelCase((P, P, B), (36, 16, 10), True, 2, (1, 0, 1)),
    ModelCase((B, B, B), (9, 8, 7), False, 2, (0, 0, 0)),
]


def case_id(c):
    tag = "".join(t[0] for t in c.topology) + "-" + "x".join(str(n) for n in c.size)
    if hasattr(c, "kind"):
        return f"{c.path}-{tag}-kind{c.kind}" + ("-regular" if c.kind == 1 and not c.stretched else "")
    return tag + ("-stretched" if c.stretched else "") + f"-{c.ntracers}tracers"


def z_of(c):
    """the z argument of the grid constructors: stretched faces, or the unit interval the helpers use for the topology"""
    if c.stretched:
        return tanh_faces(c.size[2])
    return (-1.0, 0.0) if c.topology[2] == B else (0.0, 1.0)


def z_faces_of(c):
    return np.asarray(tanh_faces(c.size[2])) if c.stretched else None


def seed_of(c):
    """one seed per case, a function of the case alone"""
    return 1000 * c.size[0] + 10 * c.size[1] + c.size[2] + 7 * sum(ord(t[0]) for t in c.topology) + getattr(c, "kind", 0)


# ---------------------------------------------------------------------------------------------------------------------
# what the host test and the GPU test both do with a case
# ---------------------------------------------------------------------------------------------------------------------
def oracle_grid(oracle, c):
    return oracle.Grid(c.size, topology=tuple(ORACLE_TOPO[t] for t in c.topology), x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(c))


def assert_same_metrics(geom, dc, df, Hz):
    """the reference's float64 z spacings are the grid's, bit for bit (dc, df: the grid's arrays, index 1 at position Hz)"""
    Nz = geom.N[2]
    assert np.array_equal(np.asarray(geom.dzc, dtype=np.float64), np.asarray(dc)[Hz:Hz + Nz])
    assert np.array_equal(np.asarray(geom.dzf[1:Nz], dtype=np.float64), np.asarray(df)[Hz + 1:Hz + Nz])


def white_noise_parents(oracle, g_cpu, seed):
    """standard-normal numbers on the whole parents of u, v, w; halos (and the impenetrable walls) filled by the oracle"""
    rng = np.random.default_rng(seed)
    A = []
    for loc in "uvw":
        a = np.asfortranarray(rng.standard_normal(g_cpu.parent_size(oracle.LOC[loc])))
        g_cpu.fill_halo_regions(a, oracle.LOC[loc])
        A.append(a)
    return A


def white_noise_interiors(geom, case):
    """standard-normal interiors of u, v, w and the tracers; wall faces of Bounded directions zero (impenetrable)"""
    rng = np.random.default_rng(seed_of(case))
    vals = {}
    for d, (name, loc) in enumerate((("u", "fcc"), ("v", "cfc"), ("w", "ccf"))):
        shape = tuple(geom.N[q] + (1 if q == d and geom.topo[q] == "Bounded" else 0) for q in range(3))
        a = rng.standard_normal(shape)
        if geom.topo[d] == "Bounded":
            a[tuple(slice(0, 1) if q == d else slice(None) for q in range(3))] = 0.0
            a[tuple(slice(-1, None) if q == d else slice(None) for q in range(3))] = 0.0
        vals[name] = a
    for t in range(case.ntracers):
        vals["c%d" % t] = rng.standard_normal(geom.N)
    return vals


def oracle_projection(oracle, g_cpu, geom, case):
    """the oracle model's projection of the case's white noise, measured against the long-double projection: errors of u, v, w, the
    long-double divergence of the oracle's and of the reference's projected fields (relative to max |∇·u0|), and the pieces the GPU test reuses"""
    vals = white_noise_interiors(geom, case)
    parents = []
    for n in "uvw":
        a = g_cpu.zeros(oracle.LOC[n])
        g_cpu.interior(a, oracle.LOC[n])[...] = vals[n]
        g_cpu.fill_halo_regions(a, oracle.LOC[n])
        parents.append(a)
    weighted = not geom.z_regular
    R = PR.source_term(geom, *parents, weighted)
    p_ref = PR.solve(R, geom, weighted)
    PR.certify(p_ref, R, geom, weighted)
    ref = dict(zip("uvw", PR.project(geom, *parents, p_ref)))
    div0 = float(np.abs(PR.source_term(geom, *parents, False)).max())
    div_ref = float(np.abs(_divergence_of_interiors(geom, ref)).max()) / div0
    m_cpu = oracle.Model(g_cpu, case.ntracers)
    m_cpu.set(enforce_incompressibility=True, **vals)
    got = {n: m_cpu.field(n).copy() for n in "uvw"}
    err = {n: PR.rel_err(geom.interior(got[n], loc), ref[n]) for n, loc in (("u", "fcc"), ("v", "cfc"), ("w", "ccf"))}
    div = float(np.abs(PR.source_term(geom, got["u"], got["v"], got["w"], False)).max()) / div0
    p_err = PR.rel_err(g_cpu.interior_cells(m_cpu.field("p")), p_ref)
    return dict(vals=vals, ref=ref, p_ref=p_ref, err=err, p_err=p_err, div=div, div_ref=div_ref, div0=div0)


def _divergence_of_interiors(geom, U):
    """∇·U of long-double interiors (N + 1 faces in Bounded directions, N wrapped in Periodic ones)"""
    out = np.zeros(geom.N, dtype=PR.LD)
    for d, n in enumerate("uvw"):
        if geom.topo[d] == "Flat":
            continue
        A = U[n]
        up = np.roll(A, -1, axis=d) if geom.topo[d] == "Periodic" else A[tuple(slice(1, None) if q == d else slice(None) for q in range(3))]
        lo = A if geom.topo[d] == "Periodic" else A[tuple(slice(0, -1) if q == d else slice(None) for q in range(3))]
        dc = geom.spacing(d)[0]
        shape = [1, 1, 1]
        shape[d] = -1
        out += (up - lo) / dc.reshape(shape)
    return out
