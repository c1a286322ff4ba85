"""The cases of test_gpu_line_kernels_in_flight.py and the one function that solves them, shared with the generator of the recorded solutions
(make_line_kernel_golden.py).

The LDS line kernels (strided_line_fft_kernel along y, zline_solve_kernel along z) pick an instantiation by line length: 8 and 16 points take
the generic loops (fewer points than k-rows per pass), 32 .. 512 the fixed-length form with 1 .. 16 elements per thread at 8 lines per
workgroup, 512 and 1024 the 4-lines-per-workgroup form with 8 and 16. Every length runs along y and along z in turn, the other directions at
8 or 16: Nx = 8 and 16 give Nxh = 5 and 9 columns of the half spectrum in rows padded to 8 and 16 -- dead lanes beside live ones, and a
partial second group of 8 lines. One (Periodic, Periodic, Bounded) stretched case runs the shared y kernel in front of the tridiagonal solve.

The solve is the model's own pressure step: set!(model; enforce_incompressibility = true) on white noise with Δt = 1, whose pNHS is the
solution of the split form (poisson_cases.py)."""
import os

import numpy as np

import poisson_reference as PR
from poisson_cases import ModelCase, P, B, case_id, white_noise_interiors, z_faces_of, z_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH_KEYS = ("split_solve_active", "fused_zfft_active")


def _ppp(size):
    return ModelCase((P, P, P), size, False, 0, (1, 1))


CASES = [
    # along y
    _ppp((8, 8, 8)), _ppp((16, 16, 8)), _ppp((8, 32, 16)), _ppp((16, 64, 8)), _ppp((16, 128, 8)), _ppp((8, 256, 8)), _ppp((16, 512, 8)), _ppp((8, 1024, 8)),
    # along z
    _ppp((16, 8, 16)), _ppp((16, 8, 32)), _ppp((8, 16, 64)), _ppp((8, 8, 128)), _ppp((16, 8, 256)), _ppp((8, 8, 512)), _ppp((8, 8, 1024)),
    # the y kernel in front of the tridiagonal solve
    ModelCase((P, P, B), (16, 64, 10), True, 0, (1, 0)),
]


def golden_path(case):
    return os.path.join(GOLDEN, "line_kernels_" + case_id(case) + ".npy")


def geometry(case):
    return PR.Geometry(case.size, case.topology, z_faces_of(case))


def solve_on_model(ocn, arch, case):
    """pNHS (interior) after the projection of the case's seeded white noise, and the model's path keys"""
    geom = geometry(case)
    grid = ocn.RectilinearGrid(arch, size=case.size, x=(0.0, 1.0), y=(0.0, 1.0), z=z_of(case), topology=tuple(getattr(ocn, t) for t in case.topology))
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=())
    paths = tuple(model.get_option(k) for k in PATH_KEYS)
    vals = white_noise_interiors(geom, case)
    ocn.set_model(model, enforce_incompressibility=True, **{n: vals[n] for n in "uvw"})
    p = np.array(geom.interior(model.pressures.pNHS.parent(), "ccc"))
    model.close()
    return p, paths
