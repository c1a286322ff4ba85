"""The cases of test_gpu_dist_line_kernels.py and the one function that solves them, shared with the generator of the recorded solutions
(make_dist_line_kernel_golden.py).

The distributed solvers run the LDS line FFTs on their run-time-length loops (ocn_line_fft.h: lds_fft_forward / lds_fft_inverse) at every
line length:

  * x-fastest substructured solve (dist_poisson_layout 4), (8, 8, Nz): source_paired_zline_r2c_kernel and paired_zline_c2r_kernel on the
    interleaved layout, Nz = 8 (odd log2: a radix-2 stage), 16 (even), 32, 256, 512 at 4 lines per workgroup and at 8 (model option
    line_zl512), 1024; Nz = 16 and 512 also with dist_fuse_source = 0, which runs paired_zline_r2c_kernel itself instead of its fused twin.
    32 pairs of columns: 4 or 8 workgroups.
  * transposing solver (dist_substructured = 0, layout -1), (Nx, 8, 8): xline_solve_kernel on the contiguous-line layout, Nx = 8 (log2 3,
    512 lines per workgroup and 40 lines in all: dead lines beside live ones), 16, 32, 64, 1024 (4 lines per workgroup, 10 workgroups).

One rank that is its own neighbour over RCCL; one RK3 step from the analytic state of the distributed tests is three pressure solves; the
interior of pNHS is what is recorded."""
import collections
import ctypes as C
import os

import numpy as np

from dist_worker import analytic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# library: options in force when the model is created; model: set on the model afterwards; paths: what the model must report
DistLineCase = collections.namedtuple("DistLineCase", "size library model paths")


def _zcase(nz, fuse=1, zl512=None):
    model = () if zl512 is None else (("line_zl512", zl512),)
    paths = (("dist_poisson_layout", 4), ("fused_step", 1), ("dist_fuse_source", fuse), ("line_zl512", 4 if zl512 is None else zl512))
    return DistLineCase((8, 8, nz), (("dist_fuse_source", fuse),), model, paths)


def _xcase(nx):
    return DistLineCase((nx, 8, 8), (("dist_substructured", 0),), (), (("dist_poisson_layout", -1), ("fused_zfft", 1)))


CASES = [_zcase(8), _zcase(16), _zcase(32), _zcase(256), _zcase(512), _zcase(512, zl512=8), _zcase(1024), _zcase(16, fuse=0), _zcase(512, fuse=0),
         _xcase(8), _xcase(16), _xcase(32), _xcase(64), _xcase(1024)]


def case_id(case):
    return "x".join(str(n) for n in case.size) + "".join(f"_{k}_{v}" for k, v in case.library + case.model if (k, v) != ("dist_fuse_source", 1))


def golden_path(case):
    return os.path.join(GOLDEN, "dist_line_kernels_" + case_id(case) + ".npy")


def solve_on_model(ocn, arch, case):
    """pNHS (interior) after one RK3 step of the one-rank self-loop model from the analytic state, and the model's path options"""
    from oldoceananigans_jl_amd import _lib, distributed as dist
    _lib.check(_lib.lib().ocn_own_stream())
    for k, v in case.library:
        ocn.set_option(k, v)
    try:
        uid = C.create_string_buffer(128)
        _lib.check(_lib.lib().ocn_dist_unique_id(uid))
        ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
        grid = dist.DistributedRectilinearGrid(ctx, size=case.size, x=(0.0, 2.0), y=(0.0, 1.0), z=(0.0, 1.0),
                                               topology=(ocn.Periodic, ocn.Periodic, ocn.Periodic))
        model = dist.LibraryDistributedModel(grid=grid, tracers=("T", "S"))
        for k, v in case.model:
            model.set_option(k, v)
        paths = tuple((k, model.get_option(k)) for k, _ in case.paths)
        ocn.set_model(model, **{n: analytic(n, *grid.global_nodes(f.loc)) for n, f in model.fields().items()})
        ocn.time_step(model, 0.1 * min(2.0 / case.size[0], 1.0 / case.size[1], 1.0 / case.size[2]) / 0.6)
        p = np.array(model.pressures.pNHS.parent()[3:-3, 3:-3, 3:-3])
        model.close()
        ctx.close()
    finally:
        for k, _ in case.library:
            ocn.set_option(k, 1)                        # the library's default of both keys
    return p, paths
