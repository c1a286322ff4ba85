"""GPU: a destroyed Poisson solver gives its device memory back. One cycle creates and destroys every solver configuration of the list
below (the serial solvers with and without the fused z transform / the split (x, y) transforms, the per-direction solver of a triply
Bounded grid, and every layout of ocn_dist_poisson_create on one rank); five cycles run. rocFFT fills caches of its own during the first
cycles, so free device memory after cycle 5 is compared with free memory after cycle 2: the loss must stay below the bytes of ONE dense
real right-hand side of the grid (Nx*Ny*Nz*8). Every solver buffer is at least that large and three cycles lie in between, so one buffer
leaked per cycle loses at least three times the bound."""
import contextlib
import ctypes as C

import pytest

from helpers import tanh_faces

pytestmark = pytest.mark.gpu

N = 64
CYCLES, BASE = 5, 2


@contextlib.contextmanager
def _defaults(ocn, opts):
    """library defaults for the solvers created inside; every key used here defaults to 1 (csrc/ocn_options.h)"""
    assert set(opts) <= {"fused_zfft", "split_solve", "dist_xfast", "dist_zfirst", "dist_substructured"}
    try:
        for k, v in opts.items():
            ocn.set_option(k, v)
        yield
    finally:
        for k in opts:
            ocn.set_option(k, 1)


def _dist_create_destroy(L, _lib, grid):
    h = C.c_void_p()
    _lib.check(L.ocn_dist_poisson_create(C.byref(h), grid.handle, 1, 0, grid.Lx))
    layout = C.c_int(-9)
    _lib.check(L.ocn_dist_poisson_layout(h, C.byref(layout)))
    _lib.check(L.ocn_dist_poisson_destroy(h))
    return layout.value


def test_destroyed_solvers_return_their_device_memory(ocn, arch):
    import torch          # (tests/conftest.py has imported it before the library was loaded)
    from oldoceananigans_jl_amd import _lib
    L = _lib.lib()
    P, B = ocn.Periodic, ocn.Bounded

    def grid(size, topology, stretched=False):
        z = tanh_faces(size[2]) if stretched else (0.0, 1.0)
        g = ocn.RectilinearGrid(arch, size=size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=topology)
        g.handle            # the device view of the grid exists before anything is measured
        return g
    ppp = grid((N, N, N), (P, P, P))
    ppp_y48 = grid((N, 48, N), (P, P, P))
    ppb = grid((N, N, N), (P, P, B), stretched=True)
    ppb_y48 = grid((N, 48, N), (P, P, B), stretched=True)
    bbb = grid((N, N, N), (B, B, B))

    def serial(cls, g):
        def run():
            cls(g).close()
        return run

    def dist(g, want):
        def run():
            layout = _dist_create_destroy(L, _lib, g)
            assert layout in want, (layout, want)
        return run
    # (options, create + destroy): the layouts are those ocn_dist_poisson_layout documents; 1 stands where the LDS y-line kernel or the 2-D
    # (y, z) plan may be refused at creation in favour of the 1-D plans
    configurations = [
        ({"fused_zfft": 1}, serial(ocn.FFTBasedPoissonSolver, ppp)),
        ({"fused_zfft": 0}, serial(ocn.FFTBasedPoissonSolver, ppp)),
        ({"split_solve": 1}, serial(ocn.FourierTridiagonalPoissonSolver, ppb)),
        ({"split_solve": 0}, serial(ocn.FourierTridiagonalPoissonSolver, ppb)),
        ({}, serial(ocn.FFTBasedPoissonSolver, bbb)),
        ({"dist_xfast": 1}, dist(ppp, (4,))),
        ({"dist_xfast": 0}, dist(ppp, (3, 1))),
        ({"dist_xfast": 0}, dist(ppp_y48, (2, 1))),
        ({"dist_xfast": 0, "dist_zfirst": 0}, dist(ppp, (0,))),
        ({"dist_substructured": 0}, dist(ppp, (-1,))),
        ({}, dist(ppb, (-1,))),
        ({}, dist(ppb_y48, (-1,))),
    ]
    fallbacks = L.ocn_debug_fft_fallbacks()
    free = []
    for _cycle in range(CYCLES):
        for opts, run in configurations:
            with _defaults(ocn, opts):
                run()
        _lib.check(L.ocn_sync())
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    lost = free[BASE - 1] - free[CYCLES - 1]
    bound = N * N * N * 8
    print("free device memory after each cycle:", free, "lost between cycle %d and %d:" % (BASE, CYCLES), lost, "bound", bound)
    assert L.ocn_debug_fft_fallbacks() == fallbacks, "a solver took the per-direction fallback: the intended paths were not the ones built"
    assert lost < bound, (free, lost, bound)
