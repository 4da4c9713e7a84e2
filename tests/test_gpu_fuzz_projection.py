"""tools/fuzz_projection.py inside the suite: random LPs with n, m in [1, 400] (either side the long one), m_eq in
{0, 1, m // 3, m - 1, m}, rows of 1 to 12 entries, one-sided, fixed and unbounded rows, variables without bounds, with and without a
starting point, through DeviceBlocks (plain and Jacobi) and DeviceADMM2, the form of the projection forced or not, on strip copies
and on the CSR kernels -- a draw of one iteration inside the error bound of one projection and at the residual bar, a longer one
iterate by iterate against the exact reference of tests/blocks_cpu.py.  tests/test_blocks_cpu_host.py checks without a GPU that
this seed keeps four fifths of its draws and reaches every branch.  A failure names seed, case and the draw."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_projection  # noqa: E402

pytestmark = pytest.mark.gpu


def test_randomised_lps_through_the_projection_solvers():
    counts = fuzz_projection.run(fuzz_projection.TEST_CASES, fuzz_projection.TEST_SEED, verbose=True)
    print(counts)
    assert counts["cases"] == fuzz_projection.TEST_CASES == 24 and counts["one_projection"] > 0
    assert 5 * counts["redraws"] <= counts["cases"] + counts["redraws"]
