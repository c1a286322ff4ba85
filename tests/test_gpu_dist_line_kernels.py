"""The LDS line kernels of the distributed Poisson solvers at every line length that takes another path through the run-time-length
transforms (dist_line_kernel_cases.py): the paired z kernels and the fused source kernel of the x-fastest substructured solve, and
xline_solve_kernel of the transposing solver.

Bit-identity with the parent of the commit that left one implementation of the line FFTs: the shared butterflies and stage bodies run the
same operations on the same values in the same order as the copies they replace, so the pressure of every case equals, bit for bit, the one
the parent's build solved for on the MI355X (tests/golden/dist_line_kernels_*.npy, written by make_dist_line_kernel_golden.py). The model's
path options are asserted too: a case that took another solver fails."""
import numpy as np
import pytest

from dist_line_kernel_cases import CASES, case_id, golden_path, solve_on_model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bit_identical_to_the_parent(ocn, arch, case):
    p, paths = solve_on_model(ocn, arch, case)
    assert paths == case.paths, (paths, case.paths)
    golden = np.load(golden_path(case))
    assert golden.shape == p.shape and golden.dtype == p.dtype
    differing = int(np.count_nonzero(golden != p))
    print(f"{case_id(case):36s} differing values: {differing} of {p.size}")
    assert np.all(np.isfinite(p))
    assert np.array_equal(golden, p)
