"""Which test runs the second path of every tuning option (csrc/ocn_api.hip: kOptions). Plain data: tests/test_options.py checks on the
CPU that the keys below are exactly the keys of kOptions -- a new option without a row fails there -- and the GPU tests take their values
from here. One entry per key, one of

    values(default, v1, v2, ...)   the non-default values that tests/test_gpu_option_variants.py (single GPU) or the preset rows of
                                   tests/test_gpu_dist_library.py (partitioned keys) run against the oracle
    covered_by("file::test")       an existing test that already runs a non-default value
    one_path("reason")             the key has no second path to test

The two grids of the tendency cases have Nz = 20 and Nz = 14: the chunk lengths are {1, 2, 3, 5, 7, Nz - 1, Nz, Nz + 1, 64} of both; the
marching epilogue runs on Nz = 12."""


def values(default, *vals):
    return {"default": default, "values": tuple(vals)}


def covered_by(node):
    return {"test": node}


def one_path(reason):
    return {"reason": reason}


CHUNKS = (1, 2, 3, 5, 7, 13, 14, 15, 19, 20, 21, 64)

VARIANTS = {
    "tendency_impl": covered_by("test_gpu_parity.py::test_tendencies_match_oracle"),
    "arithmetic": covered_by("test_gpu_arithmetic_mode.py::test_ten_steps_stay_within_1e12_of_the_oracle"),
    "role_kchunk": values(0, *CHUNKS),
    "role_ldspad": values(0, 16384),
    "fused_ty": values(7, 3),
    "fused_kchunk": values(0, *CHUNKS),
    "fused_zwin": values(1, 0),
    "fused_xcd": values(0, 1),
    "epilogue_march": covered_by("test_gpu_fullsize.py::test_marching_epilogue_equals_the_one_thread_per_value_epilogue"),
    "epilogue_rows": values(4, 1, 2, 3, 8),
    "epilogue_kchunk": values(0, 1, 2, 3, 12, 13),
    "amd_march": covered_by("test_gpu_fullsize.py::test_marching_amd_kernel_equals_the_per_cell_kernel_at_config2_size"),
    "smag_march": covered_by("test_gpu_smagorinsky.py::test_eddy_viscosity_is_the_restatement_bit_for_bit"),
    "fused_halo": covered_by("test_gpu_parity.py::test_one_launch_fill_on_bounded_z_with_boundary_conditions"),
    "real_fft": values(1, 0),
    "c2r_strided": values(1, 0),
    "fused_zfft": values(1, 0),
    "split_solve": covered_by("test_gpu_parity.py::test_split_pressure_step_equals_library_plans"),
    "line_zl512": values(4, 8),
    "skip_stage_pressure": covered_by("test_gpu_parity.py::test_stage_pressures_that_nothing_can_read_are_not_stored"),
    "skip_dead_tendency_store": covered_by("test_gpu_parity.py::test_the_tendency_after_the_second_stage_is_not_stored_and_nobody_can_tell"),
    "dist_substructured": covered_by("test_gpu_dist_library.py::test_library_self_loop_over_rccl_equals_single_gpu"),
    "dist_zfirst": covered_by("test_gpu_distributed.py::test_substructured_solver_layouts"),
    "dist_xfast": covered_by("test_gpu_dist_library.py::test_library_x_solve_layouts_agree"),
    "dist_yline": values(1, 0),
    "dist_fuse_source": covered_by("test_gpu_dist_library.py::test_fused_source_term_and_z_transform_is_bit_identical"),
    "dist_xline_group": values(1, 0),
    "dist_pencil_transposes": covered_by("test_gpu_dist_library.py::test_library_pencil_models_take_the_transposing_solver"),
    "swap_tendencies": values(1, 0),
    "fuse_substep": covered_by("test_gpu_parity.py::test_fused_substep_is_bit_identical_to_separate_kernels"),
    "fused_epilogue": covered_by("test_gpu_parity.py::test_fused_epilogue_is_bit_identical_to_separate_kernels"),
    "fused_forcing": covered_by("test_gpu_forcing.py::test_role_kernel_and_standalone_forcing_agree_over_rk3_steps"),
    "use_graph": covered_by("test_gpu_parity.py::test_time_step_graph_replay_is_bit_identical"),
    "async_halos": covered_by("test_gpu_dist_library.py::test_library_virtual_ranks_match_single_gpu"),
    "thin_halos": covered_by("test_gpu_dist_library.py::test_library_virtual_ranks_match_single_gpu"),
    "early_exchange": covered_by("test_gpu_dist_library.py::test_library_virtual_ranks_match_single_gpu"),
    "strip_width": values(0, 5),
    "fused_step": covered_by("test_gpu_dist_library.py::test_library_x_solve_layouts_agree"),
}


def default(key):
    return VARIANTS[key]["default"]


def chunk_lengths(nz):
    """the chunk lengths of the marching tendency kernels on a grid of nz levels: shorter than the three primed planes (1, 2, 3), a last
    chunk of one level (nz - 1), one chunk exactly (nz), longer than the grid (nz + 1, 64) and two lengths that leave a ragged last chunk"""
    return (1, 2, 3, 5, 7, nz - 1, nz, nz + 1, 64)
