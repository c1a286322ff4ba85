"""The kernels on either side of the pressure solve (ocn_pressure_step.h: source term, correction, dense-to-field copies) on every layout
that gives them another index map (pressure_step_cases.py): the single-GPU dense-solution path folded and unfolded, Bounded and Flat
directions, the haloed-p and complex paths, and the partitioned slab's x-fastest, z-fastest, paired-column and transposing layouts.

Bit-identity with the parent of the commit that left one divergence (source_from_faces), one correction (correct_velocities) and one dense
neighbour lookup (dense_neighbours): the shared functions run the same operations on the same values in the same order as the copies they
replace, so every recorded array of every case equals, bit for bit, what the parent's build left on the MI355X
(tests/golden/pressure_step_*.npy, written by make_pressure_step_golden.py). The model's path keys are asserted too: a case that took
another kernel fails. No value is excluded and there is no tolerance.

The z-fastest cases (10 x 34: lengths that are no power of two) run rocFFT plans whose last bits depend on the rocFFT that serves the process;
the states were recorded as this suite runs, with torch's ROCm user-space loaded first (tests/conftest.py). Every other case was recorded
both ways and is the same, bit for bit, under either."""
import numpy as np
import pytest

from pressure_step_cases import CASES, case_id, golden_path, paths_match, run_case, unpack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bit_identical_to_the_parent(ocn, arch, case):
    arrays, paths = run_case(ocn, arch, case)
    assert paths_match(paths, case.paths), (paths, case.paths)
    golden = np.load(golden_path(case))
    assert golden.dtype == np.float64 and golden.size == sum(a.size for a in arrays.values())
    want = unpack(golden, arrays)
    for n, a in arrays.items():
        differing = int(np.count_nonzero(want[n] != a))
        print(f"{case_id(case):52s} {n:5s} differing values: {differing} of {a.size}")
    for n, a in arrays.items():
        assert np.all(np.isfinite(a)), n
        assert np.array_equal(want[n], a), n
