"""``tools/fuzz_batched.run_admm_batch_stop`` inside the suite: the per-instance stopping test of the batched ADMM solver
(``k_admmb_tile`` / ``k_admmb_level`` / ``k_admmb_mult`` with ``STOP``, ``k_admmb_decide``) on batches of random small LPs -- wave /
tile / padding sizes, empty rows and columns, long rows, one- and two-sided rows, infinite and equal bounds, per-instance bounds
and starts, batches of 1 to 65 instances and one of 260.  The tolerances are the restated residual and step of one instance at a
check iteration, so that ``<=`` decides by equality.  Under six settings -- the library's own choice, both forms with a drawn
tile width from 2 to 32 and with width 64, the levels form with width 1 -- armed from creation: ``stop_state`` with
``np.array_equal`` against the numpy restatement (tests/admm_batch_stop_cpu.py) and every instance's ``x`` and ``lambda`` bit for bit
against the oracle's at that instance's own count; with the library's own choice also armed in mid-life, the chosen iteration
in its two halves, armed again with halved tolerances and turned off, and ``lp_admm_batch_until`` with its callbacks.  No instance
is left out.  tests/test_fuzz_batched_host.py checks without a GPU that this seed draws what the run claims to cover.  On a
mismatch the message names seed, case, instance, batch size, setting, form, tile width, cadence, tolerances and whether the single
solver agrees with the oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def test_randomised_batches_admm_batch_stop():
    counts = fuzz_batched.run_admm_batch_stop(CASES, SEED)
    print(counts)
    assert counts["batches"] == CASES and counts["runs"] == 6 * CASES
    assert counts["stopped"] > 0 and counts["running"] > 0 and counts["longest"] >= 260
    assert counts["mixed_tiles"] > 0 and counts["dead_tiles"] > 0
