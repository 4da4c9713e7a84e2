"""``tools/fuzz_batched.run_dga_many_stop`` inside the suite: the per-LP stopping test of dual gradient ascent on a list
(``k_dgm_iterate`` with ``STOP``) on the lists of random small LPs of the randomised cross-check -- wave / tile / padding sizes,
integer- and decimal-valued LPs, exact zeros among the costs, a list longer than the compute units.  The tolerance is the restated
step of one LP of the list at a check iteration, so that ``<=`` decides by equality.  With the launch length chosen by the library
and with one iteration per launch, armed from creation: ``stop_state`` with ``==`` against the numpy restatement
(tests/dga_stop_cpu.py) and every compared LP's x, y, tie draws and flags bit for bit against dga_cpu at that LP's own count; the
``_until`` driver on the lists without a raising LP.  Only LPs inside their parity horizon are compared; the run asserts that the
others are at most a quarter of its LPs.  tests/test_fuzz_dga_stop_host.py checks without a GPU that this seed stays within that
cap and draws stopping and running LPs side by side."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def test_randomised_lists_dual_gradient_ascent_many_stop():
    counts = fuzz_batched.run_dga_many_stop(CASES, SEED)
    print(counts)
    assert counts["lists"] == CASES and counts["runs"] == 2 * CASES
    assert counts["stopped"] > 0 and counts["running"] > 0 and counts["longest"] > 256 and counts["drivers"] > 0
    assert counts["compared"] + counts["left_out"] == counts["lps"] and 4 * counts["left_out"] <= counts["lps"]
