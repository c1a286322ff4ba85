"""The cases of test_gpu_pressure_step_kernels.py and the one function that runs them, shared with the generator of the recorded states
(make_pressure_step_golden.py).

The kernels on either side of the pressure solve (ocn_pressure_step.h) -- the source term, the correction, the copies between the dense
solution and the haloed field -- on every layout that reaches them with another index map. One RK3 step is three pressure steps.

  * single GPU, WENO, from helpers.smooth_state(1234): the parent arrays (halos included) of every prognostic field and of pNHS;
  * partitioned, one rank that is its own neighbour over RCCL, from dist_worker.analytic, built as dist_line_kernel_cases.solve_on_model
    builds its models: the interiors of u, v, w and pNHS.

What a case records is ONE float64 vector, the arrays flattened (Fortran order, the parents' own) and concatenated in the order of `names`;
what it must report is `paths`, read from the model after the step. A value of `paths` that is a tuple lists the admissible answers."""
import collections
import ctypes as C
import os

import numpy as np

from dist_worker import analytic
from helpers import smooth_state, tanh_faces

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# kind: "single" | "slab"; topology: letters of (x, y, z); z: "uniform" | "stretched"; library: options in force when the model is created;
# model: set on the model afterwards; paths: what the model must report after the step
Case = collections.namedtuple("Case", "name kind size topology z tracers library model paths")

SINGLE_KEYS = ("split_solve_active", "halo_fill_folded", "stage1_source_fused")
SLAB_KEYS = ("dist_poisson_layout", "fused_step")


def _single(name, size, topology="PPP", z="uniform", tracers=("T", "S"), model=(), paths=(1, 1, 1)):
    return Case(name, "single", size, topology, z, tracers, (), tuple(model), tuple(zip(SINGLE_KEYS, paths)))


def _slab(name, size, library=(), model=(), z="uniform", topology="PPP", paths=(4, 1)):
    return Case(name, "slab", size, topology, z, ("T", "S"), tuple(library), tuple(model), tuple(zip(SLAB_KEYS, paths)))


CASES = [
    # (5, 8, 8): H < Nx < 2H, some cells write images on both sides. Folded halos + fused stage-1 substep: substep_source_kernel and
    # pressure_correction_periodic_kernel<true, true | false>
    _single("5x8x8", (5, 8, 8)),
    # unfolded correction: pressure_correction_periodic_kernel<false, true> at stage 1, the dense correction at stages 2, 3
    _single("5x8x8_fused_halo_0", (5, 8, 8), model=[("fused_halo", 0)], paths=(1, 0, 1)),
    # source_term_kernel<true> at wrap 7, pressure_correction_periodic_kernel<true, false>
    _single("5x8x8_fuse_substep_0", (5, 8, 8), model=[("fuse_substep", 0)], paths=(1, 1, 0)),
    # the dense correction on a periodic grid at every stage
    _single("5x8x8_both_0", (5, 8, 8), model=[("fused_halo", 0), ("fuse_substep", 0)], paths=(1, 0, 0)),
    # a ragged second 64-wide block; without tracers the file stays under 512 KiB
    _single("66x8x8", (66, 8, 8), tracers=()),
    _single("66x8x8_both_0", (66, 8, 8), tracers=(), model=[("fused_halo", 0), ("fuse_substep", 0)], paths=(1, 0, 0)),
    # the no-flux rule p[0] = p[1] of the dense correction
    _single("8x8x8_ppb", (8, 8, 8), "PPB", paths=(1, 0, 0)),
    # the tridiagonal solver: weight_by_dz
    _single("8x8x8_ppb_stretched", (8, 8, 8), "PPB", "stretched", paths=(1, 0, 0)),
    # the haloed-p correction (pressure_correction_kernel) and divide_interior_kernel
    _single("8x8x8_split_solve_0", (8, 8, 8), model=[("split_solve", 0)], paths=(0, 0, 0)),
    # the complex source, source_term_kernel<false>
    _single("8x8x8_real_fft_0", (8, 8, 8), model=[("real_fft", 0)], paths=(0, 0, 0)),
    # (Periodic, Flat, Bounded): the Flat branches of the divergence and of the haloed correction
    _single("8x1x8_pfb", (8, 1, 8), "PFB", paths=(0, 0, 0)),

    # x-fastest substructured solve: source_paired_zline_r2c_kernel; the strips (columns 1..3, 6..8), then the interior range 4..5
    _slab("slab_8x8x8", (8, 8, 8)),
    # the whole slab in one launch of the column-range correction
    _slab("slab_8x8x8_early_exchange_0", (8, 8, 8), model=[("early_exchange", 0)]),
    # source_term_kernel<true> at wrap 6 with the east column
    _slab("slab_8x8x8_dist_fuse_source_0", (8, 8, 8), library=[("dist_fuse_source", 0)]),
    # z-fastest layout, the 32 x 32 tile kernels: x tiles 32 + 8, interior range 4..37 = 32 + 2; z tiles 32 + 2; y march 8 + 2
    _slab("slab_40x10x34_dist_xfast_0", (40, 10, 34), library=[("dist_xfast", 0)], paths=((1, 2, 3), 1)),
    _slab("slab_40x10x34_dist_xfast_0_early_exchange_0", (40, 10, 34), library=[("dist_xfast", 0)], model=[("early_exchange", 0)], paths=((1, 2, 3), 1)),
    # the unwrapped z-fastest source, copy_real_zfast_kernel and the ranged haloed correction
    _slab("slab_40x10x34_dist_xfast_0_fused_step_0", (40, 10, 34), library=[("dist_xfast", 0)], model=[("fused_step", 0)], paths=((1, 2, 3), 0)),
    # odd local Nx: the padded row of the paired-column layout; the strided dense copy (this layout keeps the unfused step)
    _slab("slab_9x8x8_dist_zfirst_0", (9, 8, 8), library=[("dist_zfirst", 0)], paths=(0, 0)),
    # the transposing solver: paired-column strides in the source (wrap mask 6) and in the dense correction
    _slab("slab_8x8x8_dist_substructured_0", (8, 8, 8), library=[("dist_substructured", 0)], paths=(-1, 1)),
    # ... on a Bounded stretched z: weight_by_dz, zbounded, wrap mask 2
    _slab("slab_8x8x8_dist_substructured_0_ppb_stretched", (8, 8, 8), library=[("dist_substructured", 0)], z="stretched", topology="PPB",
          paths=(-1, 1)),
]


def case_id(case):
    return case.name


def golden_path(case):
    return os.path.join(GOLDEN, "pressure_step_" + case.name + ".npy")


def paths_match(got, want):
    return len(got) == len(want) and all(k == kw and (v in vw if isinstance(vw, tuple) else v == vw) for (k, v), (kw, vw) in zip(got, want))


def time_step_of(case):
    extent = (2.0 if case.kind == "slab" else 1.0, 1.0, 1.0)
    return 0.1 * min(e / n for e, n, t in zip(extent, case.size, case.topology) if t != "F") / 0.6


def _grid_arguments(ocn, case):
    topology = tuple({"P": ocn.Periodic, "B": ocn.Bounded, "F": ocn.Flat}[t] for t in case.topology)
    nz = case.size[2]
    z = (0.0, 1.0) if case.topology[2] == "P" else (tanh_faces(nz) if case.z == "stretched" else (-1.0, 0.0))
    return topology, z


def _run_single(ocn, arch, case):
    topology, z = _grid_arguments(ocn, case)
    if "F" in case.topology:
        assert case.topology == "PFB" and case.size[1] == 1
        grid = ocn.RectilinearGrid(arch, size=(case.size[0], case.size[2]), x=(0.0, 1.0), z=z, topology=topology)
    else:
        grid = ocn.RectilinearGrid(arch, size=case.size, x=(0.0, 1.0), y=(0.0, 1.0), z=z, topology=topology)
    model = ocn.NonhydrostaticModel(grid=grid, advection=ocn.WENO(), tracers=case.tracers)
    for k, v in case.model:
        model.set_option(k, v)
    ocn.set_model(model, **smooth_state({n: grid.nodes(f.loc) for n, f in model.fields().items()}, 1234))
    ocn.time_step(model, time_step_of(case))
    paths = tuple((k, model.get_option(k)) for k, _ in case.paths)
    arrays = {n: np.array(f.parent()) for n, f in model.fields().items()}
    arrays["pNHS"] = np.array(model.pressures.pNHS.parent())
    model.close()
    return arrays, paths


def _run_slab(ocn, arch, case):
    from oldoceananigans_jl_amd import _lib, distributed as dist
    _lib.check(_lib.lib().ocn_own_stream())
    topology, z = _grid_arguments(ocn, case)
    for k, v in case.library:
        ocn.set_option(k, v)
    try:
        uid = C.create_string_buffer(128)
        _lib.check(_lib.lib().ocn_dist_unique_id(uid))
        ctx = dist.Distributed.rccl(arch, uid, 1, 0, self_loop=True)
        grid = dist.DistributedRectilinearGrid(ctx, size=case.size, x=(0.0, 2.0), y=(0.0, 1.0), z=z, topology=topology)
        model = dist.LibraryDistributedModel(grid=grid, tracers=case.tracers)
        for k, v in case.model:
            model.set_option(k, v)
        ocn.set_model(model, **{n: analytic(n, *grid.global_nodes(f.loc)) for n, f in model.fields().items()})
        ocn.time_step(model, time_step_of(case))
        paths = tuple((k, model.get_option(k)) for k, _ in case.paths)
        fields = model.fields()
        arrays = {n: np.array(fields[n].parent()[3:-3, 3:-3, 3:-3]) for n in ("u", "v", "w")}
        arrays["pNHS"] = np.array(model.pressures.pNHS.parent()[3:-3, 3:-3, 3:-3])
        model.close()
        ctx.close()
    finally:
        for k, _ in case.library:
            ocn.set_option(k, 1)                        # the library's default of every key used here
    return arrays, paths


def run_case(ocn, arch, case):
    """one RK3 step -> ({name: array} in recording order, the path keys the model reports)"""
    return (_run_single if case.kind == "single" else _run_slab)(ocn, arch, case)


def pack(arrays):
    return np.concatenate([a.ravel(order="F") for a in arrays.values()])


def unpack(vector, arrays):
    """the recorded vector cut into arrays of the names and shapes of `arrays`"""
    out, at = {}, 0
    for n, a in arrays.items():
        out[n] = vector[at:at + a.size].reshape(a.shape, order="F")
        at += a.size
    assert at == vector.size, (at, vector.size)
    return out
