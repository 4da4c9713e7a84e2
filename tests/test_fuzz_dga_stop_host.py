"""What keeps tests/test_gpu_fuzz_dga_many_stop.py from passing vacuously, checked without a GPU: under the tolerances and cadences
``tools/fuzz_batched.dga_stop_cases`` draws for ``TEST_SEED`` / ``TEST_CASES``, by the numpy restatement (tests/dga_stop_cpu.py on
dga_cpu's states), the lists hold stopping and running LPs side by side, tolerances that decide by equality, a list longer than
the compute units -- and the LPs that lie behind their parity horizon, which the GPU run cannot compare, stay within the cap of a
quarter of the run."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402

SEED, CASES = fuzz_batched.TEST_SEED, fuzz_batched.TEST_CASES


def test_the_drawn_stopping_lists_stay_within_the_cap_and_stop_and_run():
    stats = fuzz_batched.dga_stop_statistics(CASES, SEED)
    print(stats)
    assert fuzz_batched.DGA_STOP_LEFT_OUT == 0.25
    assert stats["lps"] >= CASES and stats["left_out"] <= fuzz_batched.DGA_STOP_LEFT_OUT * stats["lps"]
    assert stats["stopped"] > 0 and stats["running"] > 0 and stats["lists_with_both"] > 0
    assert stats["stopped"] + stats["running"] + stats["left_out"] == stats["lps"]
    assert stats["by_equality"] > CASES // 2 and stats["longest"] > 256


def test_a_case_is_consistent_with_its_restatement():
    import numpy as np

    import dga_stop_cpu

    cases = fuzz_batched.dga_stop_cases(CASES, SEED)
    assert len(cases) == CASES and {c.every for c in cases} <= set(fuzz_batched.DGA_STOP_EVERY)
    assert len({c.every for c in cases}) >= 3
    for case in cases:
        assert np.isfinite(case.tol) and case.tol >= 0
        if case.source is not None:
            k, t = case.source
            assert t % case.every == 0 and case.steps[k][t - 1] == case.tol and t <= case.lps[k].horizon + 1
        for lp, steps, want in zip(case.lps, case.steps, case.want):
            assert steps.size == lp.horizon + 1
            if want is None:   # left out: it does not stop inside its horizon, and the horizon does not cover the run
                assert steps.size < fuzz_batched.DGA_ITERS and dga_stop_cpu.stopping_iteration(steps, case.tol, case.every) is None
            else:
                assert want[0] <= steps.size and (want[1] or want[0] == fuzz_batched.DGA_ITERS)
