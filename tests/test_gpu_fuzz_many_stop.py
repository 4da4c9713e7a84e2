"""``tools/fuzz_batched.run_cp_many_stop`` / ``run_admm_many_stop`` inside the suite: the per-LP stopping test of the two list
solvers (``k_cpm_iterate`` / ``k_admmm_iterate`` with ``STOP``) on the lists of random small LPs of the randomised cross-check -- wave
/ tile / padding sizes, empty rows and columns, long rows, one- and two-sided rows, infinite and equal bounds, warm starts,
equality-only Chambolle-Pock LPs, a list longer than the compute units.  The tolerances are the reference step (and residual) of
one LP of the list at a check iteration, so that ``<=`` decides by equality.  Under the four settings of the list families, armed
from creation: ``stop_state`` with ``np.array_equal`` against the numpy restatements (tests/cp_stop_cpu.py, tests/admm_stop_cpu.py)
and every LP's frozen iterate bit for bit against the oracle's at that LP's own count; with the library's own choice also armed
in mid-life, the chosen iteration in its two halves, and the ``_until`` driver with its callbacks.
tests/test_fuzz_batched_host.py checks without a GPU that this seed draws stopping and running LPs of every kind side by side.
On a mismatch the message names seed, case, LP, setting, form, cadence, tolerances and whether the single solver agrees with the
oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def _assert_counts(counts):
    print(counts)
    assert counts["lists"] == CASES and counts["runs"] == 4 * CASES
    assert counts["stopped"] > 0 and counts["running"] > 0 and counts["longest"] > 256


def test_randomised_lists_chambolle_pock_many_stop():
    _assert_counts(fuzz_batched.run_cp_many_stop(CASES, SEED))


def test_randomised_lists_admm_many_stop():
    _assert_counts(fuzz_batched.run_admm_many_stop(CASES, SEED))
