"""Records tests/golden/pressure_step_<case>.npy: the state the library loaded (OCN_LIB, or the in-tree build) leaves after one RK3 step of
each case of pressure_step_cases.py. Run ON THE MI355X with the library of the commit whose bits are the yardstick:

    OCN_LIB=<that build's libocn_mi355x.so> python tests/make_pressure_step_golden.py [DIR]

The files committed were written by the parent of the commit that gave the pressure-step kernels one divergence and one correction
(float64 vectors plus a 128-byte header): from 9 KiB for (8, 1, 8) to 441 KiB for (66, 8, 8) with its halos, 3.2 MiB in all. Every case is
recorded before a path that differs from the case's is reported, so that a wrong expectation shows with the whole table beside it."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

# as tests/conftest.py does: torch brings its own ROCm user-space (hipfft / rocFFT among it) under the sonames of the system's, and whoever is
# loaded first serves the whole process. rocFFT's plans for lengths that are no power of two (the z-fastest cases: 10 x 34) differ between the two
# in the last bits, so the states are recorded with the libraries the suite runs with
if os.environ.get("OCN_TEST_NO_TORCH") != "1":
    import torch  # noqa: F401,E402
import numpy as np  # noqa: E402


def main():
    import oldoceananigans_jl_amd as ocn
    from pressure_step_cases import CASES, case_id, golden_path, pack, paths_match, run_case
    out = sys.argv[1] if len(sys.argv) > 1 else None
    arch = ocn.GPU(0)
    wrong = []
    for case in CASES:
        t0 = time.time()
        arrays, paths = run_case(ocn, arch, case)
        vector = pack(arrays)
        assert np.all(np.isfinite(vector)) and all(np.abs(a).max() > 0.0 for a in arrays.values()), case_id(case)
        path = golden_path(case) if out is None else os.path.join(out, os.path.basename(golden_path(case)))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, vector)
        ok = paths_match(paths, case.paths)
        if not ok:
            wrong.append((case_id(case), paths, case.paths))
        print(f"{case_id(case):52s} {dict(paths)} {'' if ok else 'PATHS DIFFER FROM THE CASE '}{os.path.getsize(path)} bytes, {time.time() - t0:.1f} s",
              flush=True)
    assert not wrong, wrong


if __name__ == "__main__":
    main()
