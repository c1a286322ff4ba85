"""Records tests/golden/dist_line_kernels_<case>.npy: the pressure the library loaded (OCN_LIB, or the in-tree build) solves for on each case
of dist_line_kernel_cases.py. Run ON THE MI355X with the library of the commit whose bits are the yardstick:

    OCN_LIB=<that build's libocn_mi355x.so> python tests/make_dist_line_kernel_golden.py [DIR]

The files committed were written by the parent of the commit that left one implementation of the line FFTs (float64, one value per cell,
plus a 128-byte header): from 4 KiB for (8, 8, 8) to 256 KiB for (8, 8, 512) and 512 KiB for (8, 8, 1024) and (1024, 8, 8), 2.0 MiB in all."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402


def main():
    import oldoceananigans_jl_amd as ocn
    from dist_line_kernel_cases import CASES, case_id, golden_path, solve_on_model
    out = sys.argv[1] if len(sys.argv) > 1 else None
    arch = ocn.GPU(0)
    for case in CASES:
        p, paths = solve_on_model(ocn, arch, case)
        assert paths == case.paths, (case_id(case), paths)
        assert np.all(np.isfinite(p)) and np.abs(p).max() > 0.0
        path = golden_path(case) if out is None else os.path.join(out, os.path.basename(golden_path(case)))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, p)
        print(f"{case_id(case):32s} max|p| {np.abs(p).max():.6e} -> {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
