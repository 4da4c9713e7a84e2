"""``tools/fuzz_batched.run_dga_batch_stop`` inside the suite: the per-instance stopping test of the batched dual gradient ascent
(``k_dgab_update_step``, ``k_dgab_bound_x`` / ``_y``, ``k_dgab_decide``; ``DeviceDGABatch.set_stop`` / ``stop_state``,
``dual_gradient_ascent_batch_until``) on batches of random small LPs of their own -- wave / tile / padding sizes (n <= 257, m <= 103),
integer- and decimal-valued, LPs without inequality or without equality rows, 1 to 65 instances and one batch of 260 (at most nine
distinct instances, cycled: identical data under different cut-offs), a constructed frozen instance in every third batch, 40
iterations.  The yardstick is the CPU: the step curve from dga_cpu's multipliers, the bound curve from ``dga_cpu.device_energy``, the
report's order of sums restated in numpy.  The tolerance is the restated step of one instance at a check, the cut-offs are restated
bounds of the instances' own curves (or the next float above them), so that ``<=`` and ``>=`` decide by equality.  Schedule A (armed
from creation) on the path of the parameter; schedule B (armed in mid-life, armed again with other cut-offs and another cadence,
turned off) under ``fused``.  ``stop_state`` bit for bit with dtypes against tests/dga_batch_stop_cpu.py, x, y, tie draws and flags
against dga_cpu at every instance's own count, ``report()[k, 0]`` bit for bit against ``device_energy``, the ``_until`` driver on the
batches without a raising or frozen instance.  Only instances inside their parity horizon are compared; the run asserts that the
others are at most a quarter.  tests/test_fuzz_dga_batch_stop_host.py checks without a GPU what this seed draws.

One more batch of three integer-valued instances has 65533 variables, by the general search: only from 65281 variables on does the
last of the 256 partial results of the bound's column pass hold a term, and 65536 is the most ``device_energy`` restates."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", fuzz_batched.BATCH_PATHS)
def test_randomised_batches_dual_gradient_ascent_batch_stop(path):
    counts = fuzz_batched.run_dga_batch_stop(CASES, SEED, paths=(path,))
    print(counts)
    schedules = 2 if path == "fused" else 1   # schedule B runs under fused only
    assert counts["batches"] == CASES and counts["runs"] == schedules * CASES
    assert counts["compared"] + counts["left_out"] == counts["instances"] and 4 * counts["left_out"] <= counts["instances"]
    assert counts["stopped"] > 0 and counts["running"] > 0 and counts["frozen"] > 0
    assert counts["longest"] == fuzz_batched.LONG_LIST == 260 and counts["drivers"] > 0
    assert counts["reports"] >= counts["compared"] > 0 and counts["bounds"] > 0
    assert counts["idle"] > 0 or path != "fused"


def test_the_bound_where_the_last_workgroup_of_the_column_pass_holds_terms():
    counts = fuzz_batched.run_dga_batch_stop_large(SEED)
    print(counts)
    assert counts["batches"] == 1 and counts["runs"] == 3 and counts["instances"] == 9   # A on both sorts, B under the global one
    assert counts["compared"] >= 2 and counts["stopped"] >= 2 and counts["reports"] >= 3
