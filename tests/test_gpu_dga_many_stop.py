"""The per-LP stopping test of dual gradient ascent on a list (csrc/slp_dga_many.hip: ``DeviceDGAMany.set_stop`` / ``stop_state``,
``dual_gradient_ascent_many_until``, ``solve_dga_many_until``) on the GPU.

The step is a maximum of differences a lane holds, exact in any order, and LP k of a list is bit for bit its single solve, so
everything here is compared exactly: the stopping iteration, the flag and the step (``np.array_equal``) with the numpy restatement
(tests/dga_stop_cpu.py on the states of tests/dga_cpu.py in the reference's order of sums), every stopped LP's x, y, tie draws
taken and flags with ``dga_cpu`` at that LP's own iteration, and its report with a fresh ``DeviceDGA`` run to that count.  No
tolerance appears in a comparison.  Iterates are compared inside the parity horizon the fixtures record (tests/golden/dga.npz: 100
iterations for SC105, 300 and more for the others); the steps agree in both orders of sums over all 130 iterations
(tests/test_dga_many_stop_host.py), so the stop state is compared for every LP.

The references are computed once and shared, never modified.  Needs a real MI355X: run with ``-m gpu``.
"""
import copy
import functools

import numpy as np
import pytest

import dga_stop_cpu
from conftest import load_golden, lp_from_golden
from dga_batch_cases import remainder_batch
from dga_many_cases import LP, extra_list
from test_dga_many_stop_host import FIXED_POINTS, ITERATIONS, STOPS_AT_10, TOL, expected, fifteen, fifteen_states, fifteen_steps
from test_gpu_dga_many import ListRecorder, _frozen_list, assert_lp, many_state, single_run, snapshot

pytestmark = pytest.mark.gpu

HORIZON = {12: 100}   # list index -> iterations up to which dga_cpu's reference order is the device's, where below ITERATIONS (sc105)


def _assert_stop_state(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == np.float64
    print("iterations", got[0], "expected", want[0])
    print("step", got[2], "expected", want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)


def _assert_iterates(snap, iterations, states=None, only=None):
    """LP k of the snapshot is ``dga_cpu`` after ``iterations[k]`` iterations, for every LP inside its parity horizon."""
    states = fifteen_states() if states is None else states
    for k, t in enumerate(iterations):
        if (only is not None and not only[k]) or t > HORIZON.get(k, ITERATIONS):
            continue
        assert_lp(snap, k, states[k][int(t) - 1], (k, int(t)))


@functools.lru_cache(maxsize=None)
def _single_report(k, t):
    """The report of a fresh ``DeviceDGA`` on LP ``k`` of the fifteen after ``t`` iterations (shared)."""
    _, flags, report = single_run(fifteen()[k], t)
    assert flags == 0
    return report


def _kmax_env(monkeypatch, kmax):
    if kmax is None:
        monkeypatch.delenv("SLP_DGA_MANY_KMAX", raising=False)
    else:
        monkeypatch.setenv("SLP_DGA_MANY_KMAX", str(kmax))


# ------------------------------------------------------------------ 1. stopping iterations, iterates and certified bounds
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("every", [1, 4, 10])
def test_every_lp_stops_where_the_restatement_says(monkeypatch, every, kmax):
    _kmax_env(monkeypatch, kmax)
    want = expected(TOL, every, ITERATIONS)
    assert want[1].all() and (every != 10 or tuple(want[0]) == STOPS_AT_10)
    state = many_state(fifteen())
    try:
        assert kmax is None or state.kmax() == kmax
        state.set_stop(TOL, every)
        state.iterate(ITERATIONS)
        _assert_stop_state(state.stop_state(), want)
        snap, report = snapshot(state), state.report()
    finally:
        state.close()
    _assert_iterates(snap, want[0])
    for k, t in enumerate(want[0]):   # the report of a stopped LP is the energy of its frozen multipliers: its certified bound
        assert tuple(report[k]) == _single_report(k, int(t)), (k, t)


# ------------------------------------------------------------------ 2. the split over calls
@pytest.mark.parametrize("every", [4, 10])
def test_the_split_over_calls_does_not_change_the_result(every):
    want = expected(TOL, every, ITERATIONS)
    runs = []
    for calls in ((ITERATIONS,), (1, 1, 9, 40, 79)):
        assert sum(calls) == ITERATIONS
        state = many_state(fifteen())
        try:
            state.set_stop(TOL, every)
            for k in calls:
                state.iterate(k)
            got = state.stop_state()
            _assert_stop_state(got, want)
            runs.append((got, snapshot(state), state.report()))
        finally:
            state.close()
    (_, a, ra), (_, b, rb) = runs
    for p, q in zip(a[:3], b[:3]):
        assert all(np.array_equal(u, v) for u, v in zip(p, q))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(ra, rb)


# ------------------------------------------------------------------ 3. a stopped LP is not touched
def test_a_stopped_lp_is_not_touched():
    first, more = 20, 50
    state = many_state(fifteen())
    try:
        state.set_stop(TOL, 10)
        state.iterate(first)
        state0, snap0, report0 = state.stop_state(), snapshot(state), state.report()
        _assert_stop_state(state0, expected(TOL, 10, first))
        stopped = state0[1]
        assert stopped.sum() == sum(t <= first for t in STOPS_AT_10) and 0 < stopped.sum() < 15
        state.push_random(np.random.RandomState(77).random_sample(500))   # more draws than the next call asks for
        state.iterate(more)
        state1, snap1, report1 = state.stop_state(), snapshot(state), state.report()
    finally:
        state.close()
    for k in np.flatnonzero(stopped):
        for p, q in zip(snap0[:3], snap1[:3]):
            assert np.array_equal(p[k], q[k]), k
        assert snap0[3][k] == snap1[3][k] and snap0[4][k] == snap1[4][k], k
        assert np.array_equal(report0[k], report1[k]), k
        assert all(np.array_equal(u[k], v[k]) for u, v in zip(state0, state1)), k
    # the others went on, each with its own draws of the one stream
    want = expected(TOL, 10, first + more)
    _assert_stop_state(state1, want)
    assert want[1].all() and (want[0] > first).any()
    _assert_iterates(snap1, want[0])


# ------------------------------------------------------------------ 4. tolerance 0: the exact fixed points
def test_tolerance_zero_stops_exactly_the_two_fixed_points():
    want = expected(0.0, 1, ITERATIONS)
    assert {int(k): int(want[0][k]) for k in np.flatnonzero(want[1])} == FIXED_POINTS == {5: 122, 8: 96}
    assert all(want[0][k] == ITERATIONS for k in range(15) if k not in FIXED_POINTS)
    state = many_state(fifteen())
    try:
        state.set_stop(0.0, 1)
        state.iterate(ITERATIONS)
        got = state.stop_state()
        _assert_stop_state(got, want)
        assert got[2][5] == 0.0 and got[2][8] == 0.0
        snap = snapshot(state)
    finally:
        state.close()
    _assert_iterates(snap, want[0])


# ------------------------------------------------------------------ 5. off is today
@pytest.mark.parametrize("armed_first", [False, True])
def test_without_the_test_every_lp_is_what_it_was(armed_first):
    from pysparselp_amd import dual_gradient_ascent_many

    total, armed = 60, 30
    steps = fifteen_steps()
    assert all(s[:armed].min() > 0.0 for s in steps)   # tolerance 0 at every iteration: nothing meets it in the armed part
    state = many_state(fifteen())
    try:
        if armed_first:
            state.set_stop(0.0, 1)
            state.iterate(armed)
            state.set_stop(None)
            state.iterate(total - armed)
        else:
            state.iterate(total)
        got = state.stop_state()
        last = np.array([s[armed - 1] for s in steps]) if armed_first else np.full(15, np.inf)
        _assert_stop_state(got, (np.full(15, total), np.zeros(15, dtype=bool), last))
        snap = snapshot(state)
    finally:
        state.close()
    xs, y_eqs, y_ineqs = dual_gradient_ascent_many([LP(*a) for a in fifteen()], nb_max_iter=total)
    for k in range(15):
        assert np.array_equal(snap[0][k], xs[k]) and np.array_equal(snap[1][k], y_eqs[k]), k
        assert np.array_equal(snap[2][k], y_ineqs[k] if y_ineqs[k] is not None else np.zeros(0)), k
    _assert_iterates(snap, [total] * 15)


# ------------------------------------------------------------------ 6. re-arming: no resume
def test_a_looser_tolerance_applies_to_the_moving_lps_only():
    first, fine = 40, 1e-3
    steps = fifteen_steps()
    state = many_state(fifteen())
    try:
        state.set_stop(fine, 10)
        state.iterate(first)
        before = state.stop_state()
        _assert_stop_state(before, expected(fine, 10, first))
        assert 0 < before[1].sum() < 15
        state.set_stop(TOL, 10)
        kept = state.stop_state()
        assert all(np.array_equal(u, v) for u, v in zip(before, kept))   # flags and counters stay
        state.iterate(ITERATIONS - first)
        rows = []
        for k in range(15):
            if before[1][k]:   # stays at its iteration
                rows.append((before[0][k], True, before[2][k]))
            else:              # obeys the new tolerance from the next check
                rows.append(dga_stop_cpu.stop_state(steps[k], TOL, 10, ITERATIONS, after=first, step_before=before[2][k]))
        want = tuple(np.array(col) for col in zip(*rows))
        got = state.stop_state()
        _assert_stop_state(got, want)
        assert want[1].all() and (want[0][~before[1]] == first + 10).any()
        snap = snapshot(state)
        state.set_stop(None)   # turning the test off leaves the stopped LPs stopped
        state.iterate(5)
        assert all(np.array_equal(u, v) for u, v in zip(got, state.stop_state()))
        assert state.status()[3] == snap[5]   # no LP moves: nothing was launched
    finally:
        state.close()
    _assert_iterates(snap, want[0])


# ------------------------------------------------------------------ 7. a NaN in the data
def test_an_lp_with_a_nan_in_its_cost_never_stops_and_leaves_the_others_alone():
    total = 60
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = fifteen()[1]   # random0
    c = np.array(c, copy=True)
    c[a_ineq.indices[0]] = np.nan   # a column the inequality rows meet
    others = [0, 3]
    state = many_state([(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)] + [fifteen()[k] for k in others])
    try:
        state.set_stop(TOL, 1)
        state.iterate(total)
        got = state.stop_state()
        flags = state.status()[0]
        snap = snapshot(state)
    finally:
        state.close()
    print("the LP with the NaN: iterations", got[0][0], "stopped", got[1][0], "step", got[2][0], "flags", flags[0])
    assert got[0][0] == total and not got[1][0]
    want = expected(TOL, 1, total)
    assert all(want[1][k] for k in others)
    for i, k in enumerate(others, start=1):
        assert (got[0][i], got[1][i], got[2][i]) == (want[0][k], want[1][k], want[2][k]), k
        assert_lp(snap, i, fifteen_states()[k][int(want[0][k]) - 1], k)


# ------------------------------------------------------------------ 8. a frozen LP
def test_a_frozen_lp_is_never_tested_and_the_driver_ends_without_it():
    from pysparselp_amd import dual_gradient_ascent_many_until

    problems, _ = _frozen_list()
    steps = [dga_stop_cpu.steps_of(dga_stop_cpu.states_of(problems[k], 40)) for k in (0, 2)]
    stops = [dga_stop_cpu.stopping_iteration(s, TOL, 10) for s in steps]
    assert all(t is not None for t in stops)
    state = many_state(problems)
    try:
        assert state.frozen().tolist() == [False, True, False]
        state.set_stop(TOL, 10)
        state.iterate(40)
        got = state.stop_state()
    finally:
        state.close()
    assert got[0].tolist() == [stops[0], 0, stops[1]] and got[1].tolist() == [True, False, True] and got[2][1] == np.inf
    rec = ListRecorder()
    xs, y_eqs, y_ineqs, info = dual_gradient_ascent_many_until([LP(*a) for a in problems], TOL, 10, nb_max_iter=1000, callback_func=rec)
    assert info["iterations"].tolist() == [stops[0], 0, stops[1]] and info["stopped"].tolist() == [True, False, True]
    assert rec.it == [0]   # the loop ended at the first call boundary behind the last stop, far from nb_max_iter
    assert info["lower_bound"][1] == -np.inf and np.all(np.isfinite(info["lower_bound"][[0, 2]]))


# ------------------------------------------------------------------ 9. lanes that loop, and long runs behind stopped LPs
def test_potts50_stops_by_equality_between_two_small_lps():
    """n = 7400 on 1024 lanes (npad 8192, 9800 rows): every lane loops in both update loops.  The tolerance is the LP's own
    restated step at iteration 20, so ``<=`` decides by equality; iteration 10, the check before, has a larger step."""
    total = 30
    p50 = extra_list()[3][1]
    assert p50[0].size == 7400
    steps50 = dga_stop_cpu.steps_of(dga_stop_cpu.states_of(p50, total))
    tol = float(steps50[19])
    assert steps50[9] > tol > 0.0
    small = [1, 3]
    steps = [fifteen_steps()[small[0]], steps50, fifteen_steps()[small[1]]]
    want = tuple(np.array(col) for col in zip(*[dga_stop_cpu.stop_state(s, tol, 10, total) for s in steps]))
    assert want[0][1] == 20 and want[1][1] and want[2][1] == tol
    state = many_state([fifteen()[small[0]], p50, fifteen()[small[1]]])
    try:
        state.set_stop(tol, 10)
        state.iterate(total)
        _assert_stop_state(state.stop_state(), want)
        snap, report = snapshot(state), state.report()
    finally:
        state.close()
    ref50 = dga_stop_cpu.states_of(p50, 20)
    assert_lp(snap, 1, ref50[19], "potts50")
    for i, k in ((0, small[0]), (2, small[1])):
        assert_lp(snap, i, fifteen_states()[k][int(want[0][i]) - 1], k)
    single, flags, rep = single_run(p50, 20)
    assert flags == 0 and tuple(report[1]) == rep


def test_long_runs_behind_stopped_lps_keep_the_draw_buffer_short():
    """257 LPs (one more than 256 compute units): the 65 Potts-8 LPs of the remainder batch in rotation.  Most stop at the first
    check; the run goes on well past that, one call after another, each with its refill: the draws left behind the furthest
    moving LP stay within one call's refill, and the LPs still moving get the right draws of the one stream.  Once no LP moves
    nothing is launched and nothing more is pushed: what is left is the whole window, and it stays as it is."""
    count, every, per_call, calls = 257, 5, 5, 8
    args, costs, lbs, ubs = remainder_batch()
    problems = [(costs[k % 65],) + tuple(args[1:5]) + (lbs[k % 65], ubs[k % 65]) for k in range(count)]
    total = per_call * calls
    states = [dga_stop_cpu.states_of(problems[k], total) for k in range(65)]
    rows = [dga_stop_cpu.stop_state(dga_stop_cpu.steps_of(s), TOL, every, total) for s in states]
    want = tuple(np.array([col[k % 65] for k in range(count)]) for col in zip(*rows))
    assert (want[0] == every).sum() > count // 2 and (want[0] > 2 * every).any()   # most stop at once, some much later
    state = many_state(problems)
    try:
        state.set_stop(TOL, every)
        last = int(want[0].max())
        assert every < last < total - 2 * per_call and last % per_call == 0
        offset = sum(problems[0][k].shape[0] for k in (1, 3))   # the draws of the default start: where every LP's positions begin
        still = []
        for call in range(1, calls + 1):
            state.iterate(per_call)
            _, _, left, iters = state.status()
            if call * per_call < last:   # an LP still moves
                assert 0 <= left <= 2 * per_call and iters == call * per_call, (call, left, iters)
            else:
                assert iters == last, (call, iters)
                still.append(left)
        assert len(still) >= 3 and len(set(still)) == 1 and still[0] <= offset + 2 * last + 2 * per_call, still
        _assert_stop_state(state.stop_state(), want)
        snap = snapshot(state)
    finally:
        state.close()
    for k in range(count):
        assert_lp(snap, k, states[k % 65][int(want[0][k]) - 1], k)


# ------------------------------------------------------------------ 10. the C ABI
def test_the_c_abi_refuses_a_bad_tolerance_cadence_or_handle():
    from pysparselp_amd import SlpError, _lib

    state = many_state(fifteen()[:1])
    try:
        for tol, every in ((float("nan"), 1), (float("inf"), 1), (1e-2, 0), (0.0, -1)):
            with pytest.raises(SlpError, match="slp_many_dual_set_stop"):
                _lib.check(state._l.slp_many_dual_set_stop(state._h, tol, every))
        with pytest.raises(SlpError, match="slp_many_dual_set_stop: NULL handle"):
            _lib.check(state._l.slp_many_dual_set_stop(None, 1e-2, 1))
        with pytest.raises(SlpError, match="slp_many_dual_stop_state: NULL handle"):
            _lib.check(state._l.slp_many_dual_stop_state(None, None, None, None))
        _lib.check(state._l.slp_many_dual_set_stop(state._h, -1.0, 0))   # off: the cadence is not looked at
        _lib.check(state._l.slp_many_dual_stop_state(state._h, None, None, None))
        got = state.stop_state()   # the state after create
        assert got[0].tolist() == [0] and got[1].tolist() == [False] and got[2].tolist() == [np.inf]
    finally:
        state.close()


# ------------------------------------------------------------------ 11. the drivers
class InfoRecorder(ListRecorder):
    """Also keeps the ``info`` the driver sets as an attribute of its callback, as it is at every call."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __call__(self, *report):
        super().__call__(*report)
        self.seen.append({name: values.copy() for name, values in self.info.items()})


def test_the_list_driver_ends_at_the_largest_stopping_iteration():
    from pysparselp_amd import dual_gradient_ascent_many_until

    lps = [LP(*a) for a in fifteen()]
    want = expected(TOL, 10, ITERATIONS)
    rec = InfoRecorder()
    xs, y_eqs, y_ineqs, info = dual_gradient_ascent_many_until(lps, TOL, 10, nb_max_iter=1000, callback_func=rec)
    assert sorted(info) == ["iterations", "lower_bound", "step", "stopped"]
    _assert_stop_state((info["iterations"], info["stopped"], info["step"]), want)
    assert info["iterations"].max() == max(STOPS_AT_10) == 60 and rec.it == [0]   # ended at the call boundary behind it: 100
    assert not rec.seen[0]["stopped"].any() and np.all(rec.seen[0]["iterations"] == 1)
    for k in range(15):
        ref = fifteen_states()[k][int(want[0][k]) - 1]
        assert np.array_equal(xs[k], ref[0]) and np.array_equal(y_eqs[k], ref[1]), k
        assert (y_ineqs[k] is None and ref[2] is None) or np.array_equal(y_ineqs[k], ref[2]), k
        assert info["lower_bound"][k] == _single_report(k, int(want[0][k]))[0], k
    # tolerance 0 at every iteration: two LPs stop, the run ends at nb_max_iter, and the report of index 100 sees one of them stopped
    want = expected(0.0, 1, ITERATIONS)
    rec = InfoRecorder()
    xs, _, _, info = dual_gradient_ascent_many_until(lps, 0.0, 1, nb_max_iter=ITERATIONS, callback_func=rec)
    _assert_stop_state((info["iterations"], info["stopped"], info["step"]), want)
    assert rec.it == [0, 100]
    seen = rec.seen[1]
    assert seen["stopped"].tolist() == [k == 8 for k in range(15)]
    assert seen["iterations"].tolist() == [96 if k == 8 else 101 for k in range(15)]
    assert np.array_equal(rec.x[1][8], xs[8]) and np.array_equal(xs[8], fifteen_states()[8][95][0])
    for k in range(15):
        if k != 8 and 101 <= HORIZON.get(k, ITERATIONS):
            assert np.array_equal(rec.x[1][k], fifteen_states()[k][100][0]), k


def test_solve_dga_many_until_equals_solve_for_each_lps_own_count():
    """[potts8, sc50a, random1] at ``tol = 1e-5, check_every = 10``, 201 iterations asked: by the restatement potts8 stops at 130
    (reports 0 and 100), sc50a at 70 (report 0 only) and random1 runs all 201 (reports 0, 100, 200)."""
    from pysparselp_amd import solve_dga_many_until
    from pysparselp_amd.SparseLP import SparseLP
    from test_dga_host import dga_args

    cases, tol, every, total = ("potts8", "sc50a", "random1"), 1e-5, 10, 201
    golden = [load_golden("lp_" + c) for c in cases]
    rows = [dga_stop_cpu.stop_state(dga_stop_cpu.steps_of(dga_stop_cpu.states_of(dga_args(d), total)), tol, every, total) for d in golden]
    assert [r[0] for r in rows] == [130, 70, 201] and [r[1] for r in rows] == [True, True, False]
    lps = [lp_from_golden(d, SparseLP) for d in golden]
    singles = [copy.deepcopy(lp) for lp in lps]
    xs, elapsed = solve_dga_many_until(lps, tol, check_every=every, nb_iter=total)
    assert len(xs) == 3 and elapsed > 0
    assert [lp.nb_iterations for lp in lps] == [r[0] for r in rows] and [lp.stopped for lp in lps] == [r[1] for r in rows]
    for k, (case, lp, one) in enumerate(zip(cases, lps, singles)):
        xk = one.solve(method="dual_gradient_ascent", get_timing=False, nb_iter=lp.nb_iterations)
        assert np.array_equal(xs[k], xk), case
        assert lp.itrn_curve == one.itrn_curve == list(range(0, lp.nb_iterations, 100)), case
        for name in ("pobj_curve", "dobj_curve", "max_violated_constraint", "max_violated_equality", "max_violated_inequality",
                     "distance_to_ground_truth", "distanceToGroundTruthAfterRounding", "pobjbound"):
            assert list(getattr(lp, name)) == list(getattr(one, name)), (name, case)
        assert len(lp.opttime_curve) == len(lp.dopttime_curve) == len(lp.itrn_curve)
        y_eq, y_ineq = lp.dual_multipliers
        assert y_eq.shape == (one.a_equalities.shape[0],) and isinstance(lp.dual_lower_bound, float) and np.isfinite(lp.dual_lower_bound)
