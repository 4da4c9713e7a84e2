"""``tools/fuzz_batched.run_cp_many_gap`` / ``run_cp_batch_gap`` inside the suite: the certified stopping test of the Chambolle-Pock
list solver (``k_cpm_iterate_gap``) and of the batched one (the ``k_cpb_gap_*`` kernels, the masked ``k_cpb_primal`` / ``k_cpb_dual``)
on random small LPs at the sizes their reductions can go wrong at -- n in 63, 64, 65, 127, 129, 255, 257, a row of more than 64
entries, empty rows and columns, warm starts, a list of 260 LPs, a batch of 65 -- with three LPs of four boxed, so that the bound
is finite there.  The tolerances are the violation and the relative gap (with a margin) of one LP at a check iteration.
``gap_state`` against the numpy restatement (tests/cp_gap_cpu.py): iterations and flags with ``np.array_equal`` on every LP all of
whose checks are decidable, the violation exactly, primal and bound within ``rtol = atol = 1e-9``; every frozen iterate bit for bit
against the oracle's at that LP's own count; armed in mid-life, the drawn iteration in its two halves (lists), the ``_certified``
drivers with ``info`` at every callback.  The restatement repeats the device's formula, so the recorded bound is also compared with
the formula in exact rational arithmetic on the device's own ``y`` (``cp_gap_cpu.exact_bound``) and checked to BE a lower bound
against HiGHS: no finite bound above the optimum, no feasible stopped iterate below it, ``-inf`` for ever on an unbounded LP.
tests/test_fuzz_batched_host.py checks without a GPU that this seed draws what is claimed here.  On a mismatch the message names
seed, case, LP, setting, form, cadence, tolerances and whether the single solver agrees with the oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def _assert_counts(counts, stats, runs):
    print(counts)
    assert counts["lists"] == CASES and counts["runs"] == runs * CASES
    assert counts["stopped"] > 0 and counts["running"] > 0
    assert counts["bounds_checked"] == stats["entries"] > 0 and counts["bounds_below_optimum"] > 0
    assert counts["unbounded"] > 0 and counts["infeasible"] == 0
    assert counts["stopped"] + counts["running"] + counts["left_out"] == stats["entries"]
    assert counts["left_out"] == stats["left_out"] <= fuzz_batched.GAP_LEFT_OUT * stats["entries"]
    assert counts["rounded_to_zero"] == stats["rounded_to_zero"]


def test_randomised_lists_chambolle_pock_many_gap():
    counts = fuzz_batched.run_cp_many_gap(CASES, SEED)
    _assert_counts(counts, fuzz_batched.gap_statistics(fuzz_batched.cp_gap_cases(CASES, SEED)), 4)
    assert counts["longest"] > 256


def test_randomised_batches_chambolle_pock_batch_gap():
    counts = fuzz_batched.run_cp_batch_gap(CASES, SEED)
    _assert_counts(counts, fuzz_batched.gap_statistics(fuzz_batched.cp_batch_gap_cases(CASES, SEED)), 1)
    assert counts["longest"] == fuzz_batched.CP_TILE_EDGE
