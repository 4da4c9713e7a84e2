"""What keeps tests/test_gpu_fuzz_dga_batch_stop.py from passing vacuously, checked without a GPU: under the rules
``tools/fuzz_batched.dga_batch_stop_cases`` draws for ``TEST_SEED`` / ``TEST_CASES``, by the numpy restatement
(tests/dga_batch_stop_cpu.py on dga_cpu's states and ``dga_cpu.device_energy``), every reason to stop occurs beside running
instances, tolerances and cut-offs decide by equality, every edge size, batch size and kind of LP is compared, the constructed frozen
instances sit between live ones, schedule B stops instances under both of its rules, and the instance-schedules behind their parity
horizon, which the GPU run cannot compare, stay within the cap of a quarter.  And the yardstick itself: ``device_energy`` is
``dual_energy`` up to its rounding on every state used, and exactly a plain loop over the device's layout on hand-made vectors."""
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_batched  # noqa: E402
from dga_cpu import device_energy, dual_energy  # noqa: E402

SEED, CASES = fuzz_batched.TEST_SEED, fuzz_batched.TEST_CASES


def test_the_drawn_batches_and_rules_reach_what_the_gpu_run_claims():
    stats = fuzz_batched.dga_batch_stop_statistics(CASES, SEED)
    print({name: (sorted(v) if isinstance(v, set) else int(v)) for name, v in stats.items()})
    assert fuzz_batched.DGA_STOP_LEFT_OUT == 0.25
    assert stats["instance_schedules"] == stats["compared"] + stats["left_out"] and stats["instance_schedules"] >= 2 * CASES
    assert 4 * stats["left_out"] <= stats["instance_schedules"]
    assert stats["by_step"] > 0 and stats["by_bound"] > 0 and stats["by_both"] > 0 and stats["running"] > 0
    assert stats["batches_with_both"] >= 3
    assert 3 * stats["step_by_equality"] > CASES and 3 * stats["bound_by_equality"] > CASES
    assert stats["above_not_met"] > 0
    assert {1, 64, 65, 260} <= stats["sizes"] and stats["longest"] == fuzz_batched.LONG_LIST == 260
    assert set(fuzz_batched.EDGE_N) <= stats["edge_sizes"]
    assert stats["stopped_without_ineq"] > 0 and stats["stopped_without_eq"] > 0
    assert stats["frozen_between"] >= 2 and stats["frozen"] >= stats["frozen_between"]
    assert stats["b_first_phase"] > 0 and stats["b_second_phase"] > 0 and stats["b_survive_off"] > 0
    assert stats["twins_apart"] > 0
    assert stats["idle_batches"] > 0 and stats["driver_batches"] > 0   # what the GPU test's counts `idle` and `drivers` need


def test_a_case_is_consistent_with_its_restatement():
    cases = fuzz_batched.dga_batch_stop_cases(CASES, SEED)
    assert len(cases) == CASES and {c.every for c in cases} <= set(fuzz_batched.DGA_STOP_EVERY) and len({c.every for c in cases}) >= 3
    assert [len(c.lps) for c in cases[:9]] == list(fuzz_batched.DGA_BATCH_STOP_SIZES)
    assert [c.lps[0].args[0].size for c in cases[:10]] == list(fuzz_batched.EDGE_N)
    assert max(lp.args[0].size for c in cases for lp in c.lps) <= 257 and max(sum(lp.rows) for c in cases for lp in c.lps) <= 103
    for case in cases:
        batch = len(case.lps)
        assert len(case.distinct) == min(batch, fuzz_batched.DGA_BATCH_DISTINCT)
        assert case.tol is not None or case.targets is not None
        assert (case.tol is None) == (case.no % 5 == 4 and any(case.steps(k).size for k in range(batch)))
        assert (case.targets is None) == (case.no % 5 == 2)
        if case.source is not None:
            k, t = case.source
            assert t % case.every == 0 and case.steps(k)[t - 1] == case.tol and t <= case.lps[k].horizon + 1
            assert not case.both or case.targets[k] == case.bounds(k)[t - 1]
        for k, lp in enumerate(case.lps):
            assert case.steps(k).size == case.bounds(k).size == lp.horizon + 1
            assert case.frozen[k] == (k == case.frozen_at)
            if not case.frozen[k]:
                assert lp is case.distinct[k % len(case.distinct)]
        if case.frozen_at is not None:
            lp = case.lps[case.frozen_at]
            assert sorted(lp.states) == [-1] and case.start_bound(case.frozen_at) == -np.inf and dual_energy(*lp.args, *lp.states[-1][1:3]) == -np.inf
            twin = case.distinct[case.frozen_at % len(case.distinct)]
            assert np.array_equal(lp.args[0], twin.args[0]) and np.sum(lp.args[5] != twin.args[5]) + np.sum(lp.args[6] != twin.args[6]) == 1
        if case.targets is not None:
            assert case.targets.shape == (batch,) and not np.isnan(case.targets).any() and not np.any(case.targets == -np.inf)
            for k, (kind, t) in enumerate(case.kinds):
                if kind == "none":
                    assert case.targets[k] == np.inf
                    continue
                assert t % case.every == 0 and 1 <= t <= case.bounds(k).size
                want = {"equal": case.bounds(k)[t - 1], "above": np.nextafter(case.bounds(k)[t - 1], np.inf), "never": case.bounds(k).max() + 1.0}
                assert case.targets[k] == want[kind]
        (a1, tol1, tg1, ev1), (a2, tol2, tg2, ev2), (a3, tol3, tg3, ev3) = case.rules_b
        assert 1 <= a1 <= 9 and a1 < a2 <= 25 and a2 < a3 <= 35 and (tol3, tg3, ev3) == (None, None, 1)
        assert (tol1, ev1) == (case.tol, case.every) and tg1 is case.targets and tol2 == (None if case.tol is None else case.tol / 2)
        assert tg2 is not None and tg2 is not case.targets and ev2 in fuzz_batched.DGA_STOP_EVERY
        for name in ("A", "B"):
            want, known = case.want(name)
            for k in np.flatnonzero(known):   # what is compared is decided inside the horizon
                assert case.frozen[k] or want[0][k] <= case.steps(k).size
                assert case.frozen[k] or want[1][k] or want[0][k] == fuzz_batched.DGA_ITERS
            for k in np.flatnonzero(~known):
                assert not want[1][k] and case.steps(k).size < fuzz_batched.DGA_ITERS
            # a record written under an earlier rule of schedule B is still there at the end
            if name == "B":
                early, _ = case.want("B", case.rules_b[2][0])
                for k in np.flatnonzero(early[1]):
                    assert all(np.array_equal(e[k], w[k], equal_nan=True) for e, w in zip(early, want))


def test_the_large_case_reaches_the_last_workgroup_and_compares_an_instance():
    case = fuzz_batched.dga_batch_stop_large_case(SEED)
    n = fuzz_batched.DGA_BATCH_STOP_LARGE_N
    assert 255 * 256 < n <= 65536 and n % 256 and [lp.args[0].size for lp in case.lps] == [n] * 3 and n > 8192   # no fused search
    for name in ("A", "B"):
        want, known = case.want(name)
        print(name, [w.tolist() for w in want], known.tolist())
    want, known = case.want("A")
    assert (known & want[1]).any() and case.targets is not None   # a stopped instance is compared, and the bound is evaluated
    for k in np.flatnonzero(known):
        lp = case.lps[k]
        tail = lp.args[0][255 * 256:] + 0.0   # untouched columns keep c_bar = c: the last workgroup's terms are not all zero
        assert np.any(tail != 0) and np.isfinite(case.bounds(k)).all()


def test_device_energy_is_dual_energy_up_to_its_rounding_on_every_state_used():
    worst, seen = 0.0, 0
    for case in fuzz_batched.dga_batch_stop_cases(CASES, SEED):
        for lp in case.distinct:
            for it in range(lp.horizon + 1):
                _, y_eq, y_ineq, _ = lp.states[it]
                mine, theirs = device_energy(*lp.args, y_eq, y_ineq), dual_energy(*lp.args, y_eq, y_ineq)
                slack = lp.bound_slack(y_eq, y_ineq)
                assert abs(mine - theirs) <= slack, (lp.name, it, mine, theirs, slack)
                worst, seen = max(worst, abs(mine - theirs) / max(1.0, abs(theirs))), seen + 1
    print("device_energy against dual_energy over", seen, "states: largest relative difference", worst)
    assert seen >= CASES


def _plain_energy(cols, rows):
    """``e - yb`` of the column terms ``cols`` and the row terms ``rows`` by a plain loop over the device's layout: 256 workgroups
    of 256 lanes, term ``j`` in lane ``j % 256`` of workgroup ``j // 256``; per wave the 64-lane tree of ``wave_sum`` (lane ``i``
    adds lane ``i + off``, ``off`` = 32 .. 1), the four waves in order, then the 256 partial results in order."""
    def parts(terms):
        out = []
        for group in range(256):
            lanes = [0.0 + (float(terms[group * 256 + lane]) if group * 256 + lane < len(terms) else 0.0) for lane in range(256)]
            total = None
            for wave in range(4):
                v = lanes[64 * wave:64 * wave + 64]
                for off in (32, 16, 8, 4, 2, 1):
                    v = [v[i] + v[i + off] for i in range(off)]
                total = v[0] if total is None else total + v[0]
            out.append(total)
        return out

    e = yb = 0.0
    for pe, py in zip(parts(cols), parts(rows)):
        e += pe
        yb += py
    return e - yb


def test_device_energy_is_the_plain_loop_over_the_devices_layout():
    rng = np.random.RandomState(5)
    big = np.array([1e16, 1.0, -1e16, 3.0, 2.0 ** -30, -1.0] * 50)   # terms that cancel: the order of the sums decides the result
    vectors = ((rng.randn(257) * 100, rng.randn(103)), (big, big[::-1][:129].copy()), (rng.randn(65536), rng.randn(1000) * 1e-3),
               (np.array([-0.0]), np.array([2.5])))
    orders = set()
    for cols, rows in vectors:
        n, m = cols.size, rows.size
        # an LP whose column terms are `cols` and whose row terms are `rows`: no matrix entry (c_bar = c), lb = ub = 1 (c_bar ub = c_bar),
        # y = rows, b = 1; once as equality rows alone, once split over both kinds of rows
        for m_eq in (m, m // 2):
            a_eq = scipy.sparse.csr_matrix((m_eq, n))
            a_ineq = scipy.sparse.csr_matrix((m - m_eq, n)) if m_eq < m else None
            got = device_energy(cols, a_eq, np.ones(m_eq), a_ineq, np.ones(m - m_eq) if m_eq < m else None, np.ones(n), np.ones(n),
                                rows[:m_eq], rows[m_eq:] if m_eq < m else None)
            want = _plain_energy(cols, rows)
            assert got == want and isinstance(got, float), (n, m, m_eq, got, want)
        orders.add(want == float(np.sum(cols) - np.sum(rows)))
    assert False in orders   # the layout matters: numpy's pairwise sum of the same terms gives another number somewhere
    # c_bar == 0 and y == 0 contribute nothing, whatever the bounds: an infinite bound beside a zero reduced cost is no NaN
    zero = scipy.sparse.csr_matrix((2, 3))
    assert device_energy(np.array([0.0, 2.0, -1.0]), zero, np.array([np.inf, 1.0]), None, None, np.array([-np.inf, 1.0, 0.0]),
                         np.array([5.0, 4.0, 3.0]), np.array([0.0, 0.5]), None) == (2.0 - 3.0) - 0.5
    # an open side that the reduced cost pushes to: -inf, as dual_energy
    assert device_energy(np.array([-1.0]), scipy.sparse.csr_matrix((1, 1)), np.ones(1), None, None, np.zeros(1), np.array([np.inf]),
                         np.ones(1), None) == -np.inf
