"""The bound cut-off of dual gradient ascent on a list (csrc/slp_dga_many.hip, ``k_dgm_iterate<true, true>``:
``DeviceDGAMany.set_cutoff`` / ``stop_state_full``, ``dual_gradient_ascent_many_cutoff``, ``solve_dga_many_cutoff``) on the GPU.

The kernel's bound is the report's sum, term for term in the same lane of the same wave, and the decision compares two floats, so
everything here is compared exactly: the stopping iteration, the reason, the step and the bound (``np.array_equal``) with the numpy
restatement (tests/dga_batch_stop_cpu.py on the curves of tests/dga_many_bound_cases.py, whose bounds are ``dga_cpu.device_energy``),
every stopped LP's x, y, tie draws taken and flags with ``dga_cpu`` at that LP's own iteration -- the guard against the check's
column pass writing x or c_bar --, and its recorded bound with ``report()`` and with a fresh ``DeviceDGA`` run to that count.  No
tolerance appears in a comparison.  Where a CPU run of the iterates would not be the device's bit for bit (lists of integer-valued
LPs, whose equal breakpoints the two sorts may order differently), the curves come from a run of the same list that is never
armed -- the kernel without the test, which tests/test_gpu_dga_many.py ties to the single solver -- and the bound of every
multiplier vector it shows is still ``device_energy`` on the CPU.

The references are computed once and shared, never modified.  Needs a real MI355X: run with ``-m gpu``."""
import copy
import functools

import numpy as np
import pytest

import dga_batch_stop_cpu
import dga_many_bound_cases as cases
import dga_stop_cpu
from conftest import load_golden, lp_from_golden
from dga_cpu import device_energy
from dga_many_cases import LP, extra_list
from test_dga_many_stop_host import ITERATIONS, fifteen, fifteen_states
from test_gpu_dga_many import ListRecorder, _frozen_list, assert_lp, many_state, single_run, snapshot
from test_gpu_dga_many_stop import _assert_iterates, _kmax_env, _single_report

pytestmark = pytest.mark.gpu

TOL, INF = cases.TOL, np.inf


def _assert_full(got, want):
    assert [a.dtype for a in got] == [np.int64, bool, np.float64, np.float64, np.int32]
    print("iterations", got[0], "expected", want[0])
    print("reason", got[4], "expected", want[4])
    print("bound", got[3], "expected", want[3])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)
    assert np.array_equal(got[3], want[3], equal_nan=True)
    assert np.array_equal(got[4], want[4])


def _assert_three(three, full):
    assert np.array_equal(three[0], full[0]) and np.array_equal(three[1], full[1]) and np.array_equal(three[2], full[2], equal_nan=True)


def _run(problems, rule, calls):
    """A fresh state over ``problems`` armed with ``rule = (tol, check_every, targets)``, run through ``calls``:
    ``(stop_state_full, stop_state, snapshot, report)``."""
    state = many_state(problems)
    try:
        state.set_cutoff(*rule)
        for k in calls:
            state.iterate(k)
        return state.stop_state_full(), state.stop_state(), snapshot(state), state.report()
    finally:
        state.close()


# ------------------------------------------------------------------ 1. the fifteen: records, iterates, certified bounds
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("every", cases.EVERY)
def test_every_lp_stops_where_the_restatement_says(monkeypatch, every, kmax):
    _kmax_env(monkeypatch, kmax)
    want = cases.expected([(0, TOL, cases.targets(), every)])
    full, three, snap, report = _run(fifteen(), (TOL, every, cases.targets()), (ITERATIONS,))
    _assert_full(full, want)
    _assert_three(three, full)
    _assert_iterates(snap, want[0])   # a stopped LP has the x of the top of its last iteration, the others ran to the end
    for k in np.flatnonzero(want[1]):
        t = int(want[0][k])
        assert report[k, 0] == full[3][k], (k, t)   # the recorded bound is the report's energy, bit for bit ...
        assert tuple(report[k]) == _single_report(int(k), t), (k, t)   # ... and that of a fresh single solve run to that count


# ------------------------------------------------------------------ 2. cut-offs alone: equality, one ulp above, none
def test_cut_offs_without_a_tolerance_decide_by_equality_and_record_the_step():
    targets = cases.targets()
    want = cases.expected([(0, None, targets, 10)])
    full, three, snap, report = _run(fifteen(), (None, 10, targets), (ITERATIONS,))
    _assert_full(full, want)
    _assert_three(three, full)
    assert not (full[4] & 1).any() and np.all(np.isfinite(full[2]))   # the step is evaluated and recorded, never tested
    for k, check in cases.EQUAL.items():   # monotone curves up to there: met at that check, by equality
        if want[0][k] == check:
            assert full[3][k] == targets[k] and full[4][k] == 2, k
    assert sum(want[0][k] == check for k, check in cases.EQUAL.items()) >= 2
    for k, check in cases.ABOVE.items():   # one ulp above the bound of that check: passed
        assert full[0][k] > check and full[3][k] >= targets[k] > cases.fifteen_curves()[k][1][check - 1], k
    free = np.flatnonzero(targets == INF)
    assert np.all(full[0][free] == ITERATIONS) and np.all(np.isfinite(full[3][free])) and not full[1][free].any()
    _assert_iterates(snap, want[0])
    # with the tolerance LP 3 meets both at the same check
    both = cases.expected([(0, TOL, targets, 10)])
    assert both[4][cases.BOTH] == 3


# ------------------------------------------------------------------ 3. the split over calls
def test_the_split_over_calls_does_not_change_the_result():
    want = cases.expected([(0, TOL, cases.targets(), 4)])
    runs = [_run(fifteen(), (TOL, 4, cases.targets()), calls) for calls in ((ITERATIONS,), (1, 1, 9, 40, 79))]
    for full, three, _, _ in runs:
        _assert_full(full, want)
        _assert_three(three, full)
    (_, _, a, ra), (_, _, b, rb) = runs
    for p, q in zip(a[:3], b[:3]):
        assert all(np.array_equal(u, v) for u, v in zip(p, q))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(ra, rb)


# ------------------------------------------------------------------ 4. a stopped LP is not touched
def test_a_stopped_lp_is_not_touched():
    first, more = 40, 50
    state = many_state(fifteen())
    try:
        state.set_cutoff(TOL, 10, cases.targets())
        state.iterate(first)
        state0, snap0, report0 = state.stop_state_full(), snapshot(state), state.report()
        _assert_full(state0, cases.expected([(0, TOL, cases.targets(), 10)], total=first))
        stopped = state0[1]
        assert 3 <= stopped.sum() < 15 and (state0[4][stopped] & 2).any()
        state.push_random(np.random.RandomState(77).random_sample(500))   # more draws than the next call asks for
        state.iterate(more)
        state1, snap1, report1 = state.stop_state_full(), snapshot(state), state.report()
    finally:
        state.close()
    for k in np.flatnonzero(stopped):
        for p, q in zip(snap0[:3], snap1[:3]):
            assert np.array_equal(p[k], q[k]), k
        assert snap0[3][k] == snap1[3][k] and snap0[4][k] == snap1[4][k], k
        assert np.array_equal(report0[k], report1[k]), k
        assert all(np.array_equal(u[k], v[k]) for u, v in zip(state0, state1)), k
    want = cases.expected([(0, TOL, cases.targets(), 10)], total=first + more)
    _assert_full(state1, want)
    assert (want[0] > first).any()
    _assert_iterates(snap1, want[0])


# ------------------------------------------------------------------ 5. without cut-offs everything is what it was
def test_without_cut_offs_the_state_is_the_one_armed_through_set_stop():
    from pysparselp_amd import dual_gradient_ascent_many

    total, old_tol = 60, 1e-2
    runs = []
    for arm in ("set_stop", "set_cutoff"):
        state = many_state(fifteen())
        try:
            if arm == "set_stop":
                state.set_stop(old_tol, 10)
            else:
                state.set_cutoff(old_tol, 10)
            state.iterate(total)
            runs.append((state.stop_state_full(), state.stop_state(), snapshot(state), state.report()))
        finally:
            state.close()
    (fa, ta, a, ra), (fb, tb, b, rb) = runs
    assert all(np.array_equal(u, v) for u, v in zip(fa, fb)) and all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert np.all(fa[3] == -INF) and set(fa[4].tolist()) <= {0, 1} and fa[1].any()   # no bound is ever evaluated
    for p, q in zip(a[:3], b[:3]):
        assert all(np.array_equal(u, v) for u, v in zip(p, q))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(ra, rb)
    # a state that is never armed is dual_gradient_ascent_many
    state = many_state(fifteen())
    try:
        state.iterate(total)
        full, snap = state.stop_state_full(), snapshot(state)
    finally:
        state.close()
    assert np.all(full[0] == total) and not full[1].any() and np.all(full[2] == INF) and np.all(full[3] == -INF) and not full[4].any()
    xs, y_eqs, y_ineqs = dual_gradient_ascent_many([LP(*a) for a in fifteen()], nb_max_iter=total)
    for k in range(15):
        assert np.array_equal(snap[0][k], xs[k]) and np.array_equal(snap[1][k], y_eqs[k]), k
        assert np.array_equal(snap[2][k], y_ineqs[k] if y_ineqs[k] is not None else np.zeros(0)), k


# ------------------------------------------------------------------ 6. the rule changes while the state lives
def test_arming_late_changing_the_cut_offs_dropping_them_and_turning_the_test_off():
    rules = cases.schedule()
    state = many_state(fifteen())
    try:
        done = 0
        for i, (after, tol, targets, every) in enumerate(rules):
            state.iterate(after - done)
            done = after
            if i:   # the records at the change are those of the rules so far
                _assert_full(state.stop_state_full(), cases.expected(list(rules[:i]), total=after))
            state.set_cutoff(tol, every, targets)
        state.iterate(cases.SCHEDULE_TOTAL - done)
        full, three, snap = state.stop_state_full(), state.stop_state(), snapshot(state)
    finally:
        state.close()
    want = cases.expected(list(rules), total=cases.SCHEDULE_TOTAL)
    _assert_full(full, want)
    _assert_three(three, full)
    _assert_iterates(snap, want[0])


# ------------------------------------------------------------------ 7. shapes at which the reduction can go wrong
def _unarmed_curves(problems, total):
    """Per LP ``(steps, bounds, states)`` over ``t = 1 .. total`` from a state that is never armed, read after every iteration:
    ``states[t - 1] = (x, y_eq, y_ineq, draws)`` as ``dga_cpu`` keys them (-1: the start), the bounds ``device_energy`` of its y."""
    state = many_state(problems)
    try:
        assert not state.frozen().any()
        snaps = [snapshot(state)]
        for _ in range(total):
            state.iterate(1)
            snaps.append(snapshot(state))
        assert not np.any(snaps[-1][4])
    finally:
        state.close()
    out = []
    for k, args in enumerate(problems):
        y_ineq = (lambda s: s[2][k] if args[3] is not None else None)
        states = {t - 1: (s[0][k], s[1][k], y_ineq(s), int(s[3][k])) for t, s in enumerate(snaps)}
        steps, bounds = dga_batch_stop_cpu.curves_of(states, lambda y_eq, y_in, a=args: device_energy(*a, y_eq, y_in))
        out.append((steps, bounds, states))
    return out


def test_potts50_stops_on_its_own_bound_between_two_small_lps():
    """n = 7400 and 9800 rows: 29 column parts, then 39 row parts, seventeen rounds of four virtual blocks -- the round that holds
    the last column part and the first three row parts included; every lane loops in the iteration's own passes.  Its cut-off is
    its own restated bound at iteration 20.  (Rounds that are partly empty: the edge shapes below.)"""
    total = 30
    p50 = extra_list()[3][1]
    assert p50[0].size == 7400
    states50 = dga_stop_cpu.states_of(p50, total)
    steps50, bounds50 = dga_batch_stop_cpu.curves_of(states50, lambda y_eq, y_ineq: device_energy(*p50, y_eq, y_ineq))
    target = float(bounds50[19])
    assert bounds50[9] < target
    small = [1, 3]
    curves = cases.fifteen_curves()
    steps = [curves[small[0]][0], steps50, curves[small[1]][0]]
    bounds = [curves[small[0]][1], bounds50, curves[small[1]][1]]
    targets = np.array([INF, target, INF])
    want = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, None, targets, 10)], total)
    assert want[0].tolist() == [30, 20, 30] and want[4].tolist() == [0, 2, 0] and want[3][1] == target
    full, three, snap, report = _run([fifteen()[small[0]], p50, fifteen()[small[1]]], (None, 10, targets), (total,))
    _assert_full(full, want)
    assert_lp(snap, 1, states50[19], "potts50")
    for i, k in ((0, small[0]), (2, small[1])):
        assert_lp(snap, i, fifteen_states()[k][total - 1], k)
    _, flags, rep = single_run(p50, 20)
    assert flags == 0 and tuple(report[1]) == rep and rep[0] == full[3][1]


SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def test_edge_shapes_in_a_list_of_more_workgroups_than_compute_units():
    """Ten integer-valued LPs with n and m around 1, 64, 256 and 1024 -- a wave, a virtual block, the workgroup --, 257 of them in
    rotation.  Cut-offs alone, cadence 3: LP i's is its own bound at check 3, 6, 9 or 12."""
    total, every, count = 12, 3, 257
    # (with one variable most draws have a line search without a sign change, the method's "no crossing" status: seed 7 has none)
    base = [cases.integer_lp(n, SIZES[(i + 3) % 10], m_eq=SIZES[(i + 3) % 10] // 3, seed=7 if n == 1 else i) for i, n in enumerate(SIZES)]
    curves = _unarmed_curves(base, total)
    checks = [every * (1 + i % 4) for i in range(10)]
    targets = np.array([curves[i][1][checks[i] - 1] for i in range(10)])
    want10 = dga_batch_stop_cpu.stop_state([c[0] for c in curves], [c[1] for c in curves], [(0, None, targets, every)], total)
    assert want10[1].all() and len(set(want10[0].tolist())) >= 3
    want = tuple(np.array([col[k % 10] for k in range(count)]) for col in want10)
    full, three, snap, report = _run([base[k % 10] for k in range(count)], (None, every, np.array([targets[k % 10] for k in range(count)])),
                                     (total,))
    _assert_full(full, want)
    _assert_three(three, full)
    for k in range(count):
        assert_lp(snap, k, curves[k % 10][2][int(want[0][k]) - 1], k)
        assert report[k, 0] == full[3][k], k


@functools.lru_cache(maxsize=None)
def _tall(rows):
    return cases.integer_lp(64, rows, m_eq=0, seed=3)


def test_an_lp_whose_last_part_holds_terms_stops_on_its_bound():
    """64 variables, 65533 inequality rows: one column part and 256 row parts, the last with 253 terms."""
    total, every = 6, 2
    args = _tall(65533)
    (steps, bounds, states), = _unarmed_curves([args], total)
    target = float(bounds[3])
    want = dga_batch_stop_cpu.stop_state([steps], [bounds], [(0, None, np.array([target]), every)], total)
    assert want[1][0] and want[4][0] == 2
    t = int(want[0][0])
    full, three, snap, report = _run([args], (None, every, target), (total,))
    _assert_full(full, want)
    assert_lp(snap, 0, states[t - 1], "tall")
    assert full[3][0] == device_energy(*args, states[t - 1][1], states[t - 1][2])
    _, flags, rep = single_run(args, t)
    assert flags == 0 and rep[0] == full[3][0] and tuple(report[0]) == rep


def test_more_than_65536_rows_are_refused_with_cut_offs_only():
    from pysparselp_amd import SlpError

    state = many_state([_tall(65537)])
    try:
        with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: LP 0 has 65537 rows"):
            state.set_cutoff(None, 1, 0.0)
        with pytest.raises(SlpError, match="slp_many_dual_set_cutoff"):
            state.set_cutoff(1e-3, 1, INF)
        state.set_cutoff(1e-3, 1)   # the step alone has no such limit
        state.set_stop(1e-3, 1)
        full = state.stop_state_full()
        assert full[0].tolist() == [0] and full[3].tolist() == [-INF] and full[4].tolist() == [0]
    finally:
        state.close()


# ------------------------------------------------------------------ 8. a NaN in the data, a frozen LP
def test_an_lp_with_a_nan_in_its_cost_never_stops_under_any_cut_off():
    total = 60
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = fifteen()[1]   # random0
    c = np.array(c, copy=True)
    c[a_ineq.indices[0]] = np.nan   # a column the inequality rows meet
    others = [0, 3]
    targets = np.array([-1e300] + [cases.targets()[k] for k in others])
    full, three, snap, _ = _run([(c, a_eq, b_eq, a_ineq, b_upper, lb, ub)] + [fifteen()[k] for k in others], (TOL, 10, targets), (total,))
    print("the LP with the NaN: iterations", full[0][0], "reason", full[4][0], "step", full[2][0], "bound", full[3][0], "flags", snap[4][0])
    assert full[0][0] == total and not full[1][0] and full[4][0] == 0
    want = cases.expected([(0, TOL, cases.targets(), 10)], total=total)
    assert all(want[1][k] for k in others)
    for i, k in enumerate(others, start=1):
        assert tuple(col[i] for col in full) == tuple(col[k] for col in want), k
        assert_lp(snap, i, fifteen_states()[k][int(want[0][k]) - 1], k)


def test_a_frozen_lp_is_never_tested():
    problems, _ = _frozen_list()
    total, old_tol = 40, 1e-2
    steps, bounds = [], []
    for k in (0, 2):
        states = dga_stop_cpu.states_of(problems[k], total)
        s, b = dga_batch_stop_cpu.curves_of(states, lambda y_eq, y_ineq, a=problems[k]: device_energy(*a, y_eq, y_ineq))
        steps.append(s)
        bounds.append(b)
    targets = np.array([bounds[0][19], -1e300, INF])
    want = dga_batch_stop_cpu.stop_state([steps[0], np.zeros(total), steps[1]], [bounds[0], np.zeros(total), bounds[1]],
                                         [(0, old_tol, targets, 10)], total, frozen=[False, True, False])
    state = many_state(problems)
    try:
        assert state.frozen().tolist() == [False, True, False]
        state.set_cutoff(old_tol, 10, targets)
        state.iterate(total)
        full = state.stop_state_full()
    finally:
        state.close()
    _assert_full(full, want)
    assert full[0][1] == 0 and full[3][1] == -INF and full[4][1] == 0 and full[2][1] == INF
    assert want[1][0] and want[1][2]


# ------------------------------------------------------------------ 9. the C ABI
def test_the_c_abi_refuses_bad_cut_offs_a_bad_cadence_or_handle():
    from pysparselp_amd import SlpError, _lib

    state = many_state(fifteen()[:2])
    try:
        lib, h = state._l, state._h
        for bad in ([0.0, np.nan], [-np.inf, 0.0]):
            with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: a cut-off is a number or \\+inf"):
                _lib.check(lib.slp_many_dual_set_cutoff(h, -1.0, _lib.ptr(np.array(bad)), 1))
        good = np.array([0.0, INF])
        for tol, every in ((-1.0, 0), (1e-2, 0), (1e-2, -1)):
            with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: check_every"):
                _lib.check(lib.slp_many_dual_set_cutoff(h, tol, _lib.ptr(good), every))
        with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: check_every"):
            _lib.check(lib.slp_many_dual_set_cutoff(h, 1e-2, None, 0))
        for tol in (float("nan"), float("inf")):
            with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: tol must be finite"):
                _lib.check(lib.slp_many_dual_set_cutoff(h, tol, _lib.ptr(good), 1))
        with pytest.raises(SlpError, match="slp_many_dual_set_cutoff: NULL handle"):
            _lib.check(lib.slp_many_dual_set_cutoff(None, 1e-2, None, 1))
        with pytest.raises(SlpError, match="slp_many_dual_cutoff_state: NULL handle"):
            _lib.check(lib.slp_many_dual_cutoff_state(None, None, None, None, None))
        _lib.check(lib.slp_many_dual_set_cutoff(h, -1.0, None, 0))   # off: the cadence is not looked at
        _lib.check(lib.slp_many_dual_cutoff_state(h, None, None, None, None))
        full = state.stop_state_full()   # nothing was armed by a refused call: the state after create
        assert full[0].tolist() == [0, 0] and not full[1].any() and np.all(full[2] == INF) and np.all(full[3] == -INF) and not full[4].any()
    finally:
        state.close()


# ------------------------------------------------------------------ 10. the drivers
SUB = (0, 3, 7, 10, 13, 14)   # of the fifteen: every one of them stops by 40 under TOL, cadence 10 and the cut-offs


def test_the_list_driver_ends_behind_the_last_stop():
    from pysparselp_amd import dual_gradient_ascent_many_cutoff

    lps = [LP(*fifteen()[k]) for k in SUB]
    targets = cases.targets()[list(SUB)]
    all15 = cases.expected([(0, TOL, cases.targets(), 10)])
    want = tuple(col[list(SUB)] for col in all15)
    assert want[1].all() and want[0].max() == 40 and set(want[4].tolist()) == {1, 2, 3}
    rec = ListRecorder()
    xs, y_eqs, y_ineqs, info = dual_gradient_ascent_many_cutoff(lps, TOL, 10, nb_max_iter=1000, callback_func=rec, targets=targets)
    assert sorted(info) == ["bound", "iterations", "lower_bound", "reason", "step", "stopped"]
    _assert_full((info["iterations"], info["stopped"], info["step"], info["bound"], info["reason"]), want)
    assert rec.it == [0]   # ended at the first call boundary behind the last stop, far from nb_max_iter
    for i, k in enumerate(SUB):
        ref = fifteen_states()[k][int(want[0][i]) - 1]
        assert np.array_equal(xs[i], ref[0]) and np.array_equal(y_eqs[i], ref[1]), k
        assert info["lower_bound"][i] == info["bound"][i], k   # stopped at a check with cut-offs: the final report is that bound
    # without a tolerance, to a fixed horizon
    all15 = cases.expected([(0, None, cases.targets(), 10)], total=50)
    want = tuple(col[list(SUB)] for col in all15)
    xs, _, _, info = dual_gradient_ascent_many_cutoff(lps, None, 10, nb_max_iter=50, targets=targets)
    _assert_full((info["iterations"], info["stopped"], info["step"], info["bound"], info["reason"]), want)
    assert not want[1].all() and not (info["reason"] & 1).any()
    for i in np.flatnonzero(want[1]):
        assert info["lower_bound"][i] == info["bound"][i], i


def test_solve_dga_many_cutoff_sets_the_reason_and_the_certified_bound():
    """[potts8, sc50a, random1] at ``tol = 1e-5, check_every = 10``, 201 iterations asked: on their steps potts8 stops at 130, sc50a
    at 70 and random1 runs on; potts8's cut-off is its own restated bound at 50."""
    from pysparselp_amd import solve_dga_many_cutoff
    from pysparselp_amd.SparseLP import SparseLP
    from test_dga_host import dga_args

    names, tol, every, total = ("potts8", "sc50a", "random1"), 1e-5, 10, 201
    golden = [load_golden("lp_" + c) for c in names]
    curves = []
    for d in golden:
        args = dga_args(d)
        curves.append(dga_batch_stop_cpu.curves_of(dga_stop_cpu.states_of(args, total), lambda y_eq, y_ineq, a=args: device_energy(*a, y_eq, y_ineq)))
    targets = np.array([curves[0][1][49], INF, INF])
    want = dga_batch_stop_cpu.stop_state([c[0] for c in curves], [c[1] for c in curves], [(0, tol, targets, every)], total)
    assert want[0].tolist() == [50, 70, 201] and want[4].tolist() == [2, 1, 0]
    lps = [lp_from_golden(d, SparseLP) for d in golden]
    singles = [copy.deepcopy(lp) for lp in lps]
    xs, elapsed = solve_dga_many_cutoff(lps, tol, check_every=every, nb_iter=total, targets=targets)
    assert len(xs) == 3 and elapsed > 0
    assert [lp.nb_iterations for lp in lps] == want[0].tolist() and [lp.stopped for lp in lps] == want[1].tolist()
    assert [lp.stop_reason for lp in lps] == want[4].tolist() and all(isinstance(lp.stop_reason, int) for lp in lps)
    assert lps[0].dual_lower_bound == targets[0] == want[3][0]
    for k, (name, lp, one) in enumerate(zip(names, lps, singles)):
        xk = one.solve(method="dual_gradient_ascent", get_timing=False, nb_iter=lp.nb_iterations)
        assert np.array_equal(xs[k], xk), name
        assert lp.itrn_curve == one.itrn_curve == list(range(0, lp.nb_iterations, 100)), name
        assert isinstance(lp.dual_lower_bound, float) and np.isfinite(lp.dual_lower_bound)
