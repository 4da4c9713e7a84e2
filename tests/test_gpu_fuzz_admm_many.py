"""``tools/fuzz_batched.run_admm_many`` inside the suite: lists of random small LPs (wave / tile / padding sizes, empty rows and
columns, long rows, one- and two-sided rows, infinite and equal bounds, warm starts, odd reporting cadences) through
``lp_admm_many`` / ``ADMMManyState`` with the form chosen by the library, forced to ``lds`` and to ``global``, and with one
iteration per launch -- every LP bit for bit against ``oracle.lp_admm`` at every report and at the end.  On a mismatch the
message names seed, case, LP, setting and whether the single solver agrees with the oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def test_randomised_lists_admm_many():
    counts = fuzz_batched.run_admm_many(CASES, SEED)
    print(counts)
    assert counts["lists"] == CASES and counts["runs"] == 4 * CASES and counts["longest"] > 256
