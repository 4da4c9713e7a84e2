"""tools/fuzz_batched.py inside the suite: random small LPs with wave / tile / padding sizes, empty rows and columns, long rows,
one- and two-sided rows, infinite and equal bounds, warm starts and odd reporting cadences through the batched, list and
dual-ascent solver families -- every instance and every LP bit for bit against its CPU reference (``oracle.chambolle_pock_ppd``,
``oracle.lp_admm``, tests/dga_cpu.py) and against the single solver alone, the status bits where dga_cpu raises, and the dual bound
against HiGHS.  tests/test_fuzz_batched_host.py checks without a GPU that this seed draws what these tests need.  On a mismatch
the message names seed, case, instance / LP, form / path and whether the single solver agrees with the CPU reference."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

CASES, SEED = fuzz_batched.TEST_CASES, fuzz_batched.TEST_SEED

pytestmark = pytest.mark.gpu


def test_randomised_lps_chambolle_pock_batch():
    counts = fuzz_batched.run_cp_batch(CASES, SEED)
    print(counts)
    assert counts["batches"] == CASES and counts["instances"] > CASES and counts["equalities_only"] > 0


def test_randomised_lps_chambolle_pock_many():
    counts = fuzz_batched.run_cp_many(CASES, SEED)
    print(counts)
    assert counts["lists"] == CASES and counts["runs"] == 4 * CASES and counts["longest"] > 256 and counts["equalities_only"] > 0


def test_randomised_lps_admm_batch():
    counts = fuzz_batched.run_admm_batch(CASES, SEED)
    print(counts)
    assert counts["batches"] == CASES and counts["instances"] > CASES


def test_randomised_lps_dual_gradient_ascent():
    counts = fuzz_batched.run_dga(CASES, SEED)
    print(counts)
    assert counts["lps"] >= CASES and counts["raises"] > 0 and counts["bounds"] > 0 and counts["bounds_skipped"] == 0 and counts["comparisons"] > 2 * CASES


def test_randomised_lps_dual_gradient_ascent_batch():
    counts = fuzz_batched.run_dga_batch(CASES, SEED)
    print(counts)
    assert counts["batches"] == CASES and counts["raises"] > counts["raises_without_neighbours"] and counts["bounds"] > 0 and counts["bounds_skipped"] == 0


def test_randomised_lps_dual_gradient_ascent_many():
    counts = fuzz_batched.run_dga_many(CASES, SEED)
    print(counts)
    assert counts["lists"] == CASES and counts["longest"] > 256 and counts["raises"] > 0 and counts["bounds"] > 0 and counts["bounds_skipped"] == 0
