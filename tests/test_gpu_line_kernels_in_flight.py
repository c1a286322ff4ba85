"""The LDS line kernels at every line length that selects another instantiation (line_kernel_cases.py): the fixed-length forms that keep a
whole line's loads in flight, the generic loops below them, dead lanes and partial groups of lines.

1. Bit-identity with the parent commit: the fixed-length forms run the same operations on the same values in the same order as the generic
   loops they replace, so the pressure of every case equals, bit for bit, the one the parent's build solved for on the MI355X
   (tests/golden/line_kernels_*.npy, written by make_line_kernel_golden.py).
2. The yardstick of test_gpu_poisson_white_noise.py for the model's pressure step: the error against the certified long-double solve
   (poisson_reference.py) may be FACTOR x max(the oracle's error on the same source, eps).

Each case is solved once on the GPU; both tests read that solution."""
import numpy as np
import pytest

import poisson_reference as PR
from line_kernel_cases import CASES, case_id, geometry, golden_path, solve_on_model
from poisson_cases import oracle_grid, oracle_projection
from test_gpu_poisson_white_noise import EPS, FACTOR

pytestmark = pytest.mark.gpu

_solved = {}


def _solution(ocn, arch, case):
    if case not in _solved:
        p, paths = solve_on_model(ocn, arch, case)
        p.setflags(write=False)
        _solved[case] = (p, paths)
    return _solved[case]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bit_identical_to_the_parent(ocn, arch, case):
    p, paths = _solution(ocn, arch, case)
    assert paths == case.paths, (paths, case.paths)          # the line kernels ran: the split form, and the fused z pass where z is Periodic
    golden = np.load(golden_path(case))
    assert golden.shape == p.shape and golden.dtype == p.dtype
    differing = int(np.count_nonzero(golden != p))
    print(f"{case_id(case):36s} differing values: {differing} of {p.size}")
    assert np.array_equal(golden, p)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_within_the_white_noise_bar(ocn, oracle, arch, case):
    p, paths = _solution(ocn, arch, case)
    assert paths == case.paths, (paths, case.paths)
    out = oracle_projection(oracle, oracle_grid(oracle, case), geometry(case), case)
    p_err = PR.rel_err(p, out["p_ref"])
    print(f"{case_id(case):36s} p: err hip {p_err:.2e} oracle {out['p_err']:.2e} ratio {p_err / max(out['p_err'], EPS):5.2f}")
    assert np.all(np.isfinite(p))
    assert p_err <= FACTOR * max(out["p_err"], EPS), (p_err, out["p_err"])
