"""Dual gradient ascent on a list of LPs on the GPU (csrc/slp_dga_many.hip: one workgroup per LP, whole iterations inside a
launch): LP k of a list against tests/dga_cpu.py in the reference's order of sums and against the single-instance ``DeviceDGA``
on LP k alone -- bit for bit: x, y, the tie draws taken, the flags and the report -- for mixed shapes, more LPs than compute
units, gradient parts of more than one tile, a frozen LP, every split of the iterations over launches and calls, status flags,
and through ``dual_gradient_ascent_many`` and ``SparseLP.solve_dga_many``.  No tolerance appears in a comparison of iterates."""
import copy

import numpy as np
import pytest
import scipy.sparse

from conftest import load_golden, lp_from_golden
from dga_batch_cases import (INT_KEEP, REMAINDER_ITERS, STOPS, integer_batch, integer_states, reference_states, remainder_batch,
                             remainder_states)
from dga_cpu import dga_cpu, dual_argmin, dual_energy
from dga_many_cases import LP, extra_list, mixed_list, rows_of
from test_dga_host import dga_args
from test_gpu_dga import device_state, start_of
from test_gpu_dga_batch import _sc50a_with_an_unbounded_instance

pytestmark = pytest.mark.gpu


def many_state(problems, y_eq=None, y_ineq=None, draws=None):
    """A ``DeviceDGAMany`` over LPs given as ``dga_cpu`` takes them, each at the reference's start for its own shape."""
    from pysparselp_amd.DualGradientAscent import DeviceDGAMany, _dga_many_lp, dga_many_start

    forms = [_dga_many_lp(k, LP(*a)) for k, a in enumerate(problems)]
    y0s, offsets = dga_many_start(forms, y_eq, y_ineq)
    return DeviceDGAMany(forms, y0s, offsets, draws=draws)


def snapshot(state):
    flags, draws, _, iters = state.status()
    y_eqs, y_ineqs = state.y()
    return state.x(), y_eqs, y_ineqs, draws, flags, iters


def assert_lp(snap, k, ref, what):
    """LP k of a snapshot equals ``ref = (x, y_eq, y_ineq, draws)``."""
    x, y_eq, y_ineq, draws, flags, _ = snap
    assert flags[k] == 0, what
    assert np.array_equal(x[k], ref[0]), what
    assert np.array_equal(y_eq[k], ref[1]), what
    assert np.array_equal(y_ineq[k], ref[2] if ref[2] is not None else np.zeros(0)), what
    assert draws[k] == ref[3], what


def single_run(args, iters):
    """``(x, y_eq, y_ineq, draws), flags, report`` of a fresh ``DeviceDGA`` on the LP alone after ``iters`` iterations."""
    single, mat = device_state(args, "fused" if args[0].size <= 2048 else "general")
    try:
        single.iterate(iters)
        flags, draws, _, _ = single.status()
        return (single.x(), *single.y(), draws), flags, single.report()
    finally:
        single.close()
        mat.close()


def test_gpu_dga_many_mixed_list_matches_the_reference_lp_by_lp():
    """Twelve LPs of three shapes as ONE list, stopped after 1, 2, 11, 51, 101 iterations (calls of uneven size)."""
    lps = mixed_list()
    state = many_state([args for _, _, args in lps])
    try:
        assert state.kmax() >= 1
        done = 0
        for it in STOPS:
            state.iterate(it + 1 - done)
            done = it + 1
            snap = snapshot(state)
            assert snap[5] == done
            for k, (case, cost, _) in enumerate(lps):
                assert_lp(snap, k, reference_states(case)[cost][it], (k, case, cost, it))
    finally:
        state.close()


def test_gpu_dga_many_every_lp_equals_the_single_solver():
    """The mixed list plus SC105, an equality-only LP, an inequality-only LP and Potts-50 (npad 8192, 39 row tiles): after 101
    iterations LP k is the ``DeviceDGA`` run on it alone, and so is its report (the reductions are shared)."""
    problems = [args for _, _, args in mixed_list()] + [args for _, args in extra_list()]
    assert max(a[0].size for a in problems) == 7400 and any(rows_of(a)[0] == 0 for a in problems) and any(rows_of(a)[1] == 0 for a in problems)
    state = many_state(problems)
    try:
        state.iterate(101)
        snap = snapshot(state)
        report = state.report()
    finally:
        state.close()
    for k, args in enumerate(problems):
        ref, flags, rep = single_run(args, 101)
        assert flags == 0
        assert_lp(snap, k, ref, k)
        assert tuple(report[k]) == rep, k


@pytest.mark.parametrize("count", [1, 3, 65, 257])
def test_gpu_dga_many_more_lps_than_compute_units(count):
    """The 65 per-instance-bounds Potts-8 LPs of the batched suite as separate LPs; at 257 cyclically: one more than 256 compute
    units."""
    args, costs, lbs, ubs = remainder_batch()
    ref = remainder_states()
    problems = [(costs[k % 65],) + tuple(args[1:5]) + (lbs[k % 65], ubs[k % 65]) for k in range(count)]
    state = many_state(problems)
    try:
        state.iterate(REMAINDER_ITERS)
        snap = snapshot(state)
        for k in range(count):
            assert_lp(snap, k, ref[k % 65][REMAINDER_ITERS - 1], (count, k))
    finally:
        state.close()


def _tall_integer_lp():
    """The construction of ``integer_lp`` (tests/test_gpu_dga.py): m = 70 000 rows (274 tiles of 256: two per gradient part),
    n = 2000, 4 entries per row, 3000 equality rows."""
    m, n, k, m_eq = 70_000, 2000, 4, 3000
    rng = np.random.RandomState(31)
    cols = (np.arange(k) * (n // k) + rng.randint(0, n // k, size=(m, k))).astype(np.int32)
    vals = np.round(100 * rng.randn(m, k))
    vals[vals == 0] = 1.0
    a = scipy.sparse.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, m * k + 1, k)), shape=(m, n))
    lb = rng.randint(-5, 1, size=n).astype(np.float64)
    ub = lb + rng.randint(1, 10, size=n)
    xf = lb + np.floor(rng.rand(n) * (ub - lb + 1))
    ax = a @ xf
    b = ax + rng.randint(0, 50, size=m)
    b[:m_eq] = ax[:m_eq]
    c = np.round(100 * rng.randn(n))
    return c, a[:m_eq].tocsr(), b[:m_eq], a[m_eq:].tocsr(), b[m_eq:], lb, ub


def test_gpu_dga_many_gradient_parts_of_two_tiles_and_five_scan_tiles():
    """A 70 000-row LP between two small ones equals its single solve after 30 iterations; the n = 5000 LPs of the batched suite
    (up to five scan tiles in the fused search) equal the reference's order of sums at 1, 10 and 30 iterations."""
    small = [args for _, _, args in mixed_list()]
    tall = _tall_integer_lp()
    args, costs, lbs, ubs = integer_batch()
    ref = integer_states()
    problems = [small[0], tall, small[3]] + [(costs[k],) + tuple(args[1:5]) + (lbs[k], ubs[k]) for k in range(5)]
    state = many_state(problems)
    try:
        done = 0
        for it in INT_KEEP:
            state.iterate(it + 1 - done)
            done = it + 1
            snap = snapshot(state)
            for k in range(5):
                assert_lp(snap, 3 + k, ref[k][it], (it, k))
        report = state.report()
    finally:
        state.close()
    assert done == 30
    for k in (0, 1, 2):
        single, flags, rep = single_run(problems[k], 30)
        assert flags == 0
        assert_lp(snap, k, single, k)
        assert tuple(report[k]) == rep, k


def _frozen_list():
    args, costs, ubs, j = _sc50a_with_an_unbounded_instance()
    return [(costs[k],) + tuple(args[1:6]) + (ubs[k],) for k in range(3)], j


def test_gpu_dga_many_a_dual_infeasible_start_freezes_its_lp_only():
    from pysparselp_amd import dual_gradient_ascent_many
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    problems, j = _frozen_list()
    y_eq, y_ineq, _ = start_of(problems[1][1], problems[1][3])
    state = many_state(problems)
    try:
        assert state.frozen().tolist() == [False, True, False]
        state.iterate(50)
        snap = snapshot(state)
        assert state.report()[1, 0] == -np.inf
    finally:
        state.close()
    start = dga_cpu(*problems[1], nb_max_iter=50)
    assert sorted(start) == [-1]
    assert_lp(snap, 1, (start[-1][0], y_eq, y_ineq, 0), "frozen")
    assert snap[0][1][j] == np.inf
    for k in (0, 2):
        single, flags, _ = single_run(problems[k], 50)
        assert_lp(snap, k, single, k)
    # the function returns the start of the frozen LP
    xs, yes, yis = dual_gradient_ascent_many([LP(*a) for a in problems], nb_max_iter=50)
    for k in range(3):
        one = dual_gradient_ascent(None, LP(*problems[k]), nb_max_iter=50)
        assert np.array_equal(xs[k], one[0]) and np.array_equal(yes[k], one[1]) and np.array_equal(yis[k], one[2]), k


def test_gpu_dga_many_splits_over_launches_calls_and_refills_do_not_change_the_result(monkeypatch):
    """101 iterations as one call, as 1 + 1 + 9 + 40 + 50 with one and with seven iterations per launch, and with the draw buffer
    refilled five draws at a time (calls that stop early)."""
    problems = [args for _, _, args in mixed_list()[:8]]
    offsets = np.array([sum(rows_of(a)) for a in problems])
    runs = []
    state = many_state(problems)
    try:
        state.iterate(101)
        runs.append(snapshot(state))
    finally:
        state.close()
    for kmax in ("1", "7"):
        monkeypatch.setenv("SLP_DGA_MANY_KMAX", kmax)
        state = many_state(problems)
        try:
            assert state.kmax() == int(kmax)
            for k in (1, 1, 9, 40, 50):
                state.iterate(k)
            runs.append(snapshot(state))
        finally:
            state.close()
    monkeypatch.delenv("SLP_DGA_MANY_KMAX")
    rs = np.random.RandomState(0)
    state = many_state(problems)
    try:
        left = state.status()[2]
        assert left == -offsets.max()   # nothing on the device yet: the furthest LP starts behind its own start's draws
        state.push_random(rs.random_sample(-left))
        calls = 0
        while state.status()[3] < 101:
            state.push_random(rs.random_sample(5))
            state.iterate(101 - state.status()[3], refill=False)
            calls += 1
        assert calls >= 5
        snap = snapshot(state)
        assert np.all(snap[4] & ~4 == 0)
        runs.append(snap[:4] + (snap[4] & ~4, snap[5]))
    finally:
        state.close()
    for run in runs:
        assert not run[4].any() and run[5] == 101
    for run in runs[1:]:
        for p, q in zip(runs[0][:3], run[:3]):
            assert all(np.array_equal(u, v) for u, v in zip(p, q))
        assert np.array_equal(runs[0][3], run[3])
    assert runs[0][3].max() > 0 and len(set((offsets + runs[0][3]).tolist())) > 1   # different places of the stream


def test_gpu_dga_many_status_names_the_lp_and_the_launch_cap_is_validated(monkeypatch):
    """The all-zero inequality block of tests/test_gpu_dga.py on ONE LP of the list: the direction meets no column there."""
    from pysparselp_amd import SlpError
    from pysparselp_amd.DualGradientAscent import STATUS_EMPTY

    small = [args for _, _, args in mixed_list()]
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = small[3]   # sc50a
    empty = scipy.sparse.csr_matrix((np.zeros(6), np.array([0, 5, 1, 7, 2, 9]), np.array([0, 2, 4, 6])), shape=(3, c.size))
    problems = [small[0], (c, a_eq, b_eq, empty, np.ones(3), lb, ub), small[3]]
    state = many_state(problems)
    try:
        state.iterate(1)
        flags = state.status()[0]
        assert flags[1] & STATUS_EMPTY and flags[0] == 0 and flags[2] == 0
        with pytest.raises(ValueError, match=r"empty breakpoint set.*LPs \[1\] of the list"):
            state.check()
    finally:
        state.close()
    for bad in ("0", "abc"):
        monkeypatch.setenv("SLP_DGA_MANY_KMAX", bad)
        with pytest.raises(SlpError, match="SLP_DGA_MANY_KMAX must be a positive number"):
            many_state(problems)


class ListRecorder:
    """The callback's arguments, the iterates as the list of per-LP arrays they come as (their lengths differ)."""

    def __init__(self):
        self.it, self.x, self.rest = [], [], []

    def __call__(self, niter, sols, e1, e2, dur, veq, vineq):
        self.it.append(niter)
        self.x.append([np.array(v, copy=True) for v in sols])
        self.rest.append((e1, e2, veq, vineq))


def test_gpu_dga_many_function_callbacks_max_time_and_given_multipliers():
    from pysparselp_amd import dual_gradient_ascent_many
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent

    problems = [args for _, _, args in mixed_list()[1:4]]   # random0, random1, sc50a
    lps = [LP(*a) for a in problems]
    rec = ListRecorder()
    out = dual_gradient_ascent_many(lps, nb_max_iter=250, callback_func=rec)
    assert rec.it == [0, 100, 200] and rec.rest == [(0, 0, 0, 0)] * 3
    for it, xs in zip(rec.it, rec.x):   # the x of the top of that iteration, one array per LP
        assert len(xs) == 3
        for k, lp in enumerate(lps):
            assert np.array_equal(xs[k], dual_gradient_ascent(None, lp, nb_max_iter=it + 1)[0]), (it, k)
    for k, lp in enumerate(lps):
        one = dual_gradient_ascent(None, lp, nb_max_iter=250)
        assert np.array_equal(out[0][k], one[0]) and np.array_equal(out[1][k], one[1]) and np.array_equal(out[2][k], one[2]), k
    rec = ListRecorder()
    out = dual_gradient_ascent_many(lps, nb_max_iter=250, callback_func=rec, max_time=1e-9)   # ends at the first report
    assert rec.it == [0]
    for k, lp in enumerate(lps):
        one = dual_gradient_ascent(None, lp, nb_max_iter=1)
        assert np.array_equal(out[0][k], one[0]) and np.array_equal(out[1][k], one[1]) and np.array_equal(out[2][k], one[2]), k
    # the caller's multipliers for LP 1 (both parts: its tie draws start the stream) and for the equalities of LP 2 only
    rs = np.random.RandomState(3)
    ye = [None, rs.randn(rows_of(problems[1])[0]), rs.randn(rows_of(problems[2])[0])]
    yi = [None, rs.rand(rows_of(problems[1])[1]), None]
    out = dual_gradient_ascent_many(lps, nb_max_iter=60, y_eq=ye, y_ineq=yi)
    for k, lp in enumerate(lps):
        one = dual_gradient_ascent(None, lp, nb_max_iter=60, y_eq=ye[k], y_ineq=yi[k])
        assert np.array_equal(out[0][k], one[0]) and np.array_equal(out[1][k], one[1]) and np.array_equal(out[2][k], one[2]), k


def test_gpu_solve_dga_many_curves_solutions_and_certified_bounds():
    """[potts8, sc50a, random0], 201 iterations: solutions and curves (apart from the times) are those of each LP's own
    ``solve(method="dual_gradient_ascent")``.  ``dual_lower_bound`` is, to the bit, the report of the single solver standing at the
    returned multipliers.  Against the numpy dual energy of the same multipliers (another order of the same n + m terms) it holds
    to the bound derived in tests/test_gpu_dga_batch.py::test_gpu_solve_dga_batch_curves_solutions_and_certified_bounds:
    2 (n + m + 2) u (S_x + S_y), S_x = sum|min(c_bar ub, c_bar lb)|, S_y = sum|y_i b_i|, u = 2^-53."""
    from pysparselp_amd import solve_dga_many
    from pysparselp_amd.DualGradientAscent import DeviceDGA
    from pysparselp_amd.SparseLP import SparseLP
    from pysparselp_amd.device import DeviceMatrix

    cases = ("potts8", "sc50a", "random0")
    golden = [load_golden("lp_" + c) for c in cases]
    lps = [lp_from_golden(d, SparseLP) for d in golden]
    singles = [copy.deepcopy(lp) for lp in lps]
    xs, elapsed = solve_dga_many(lps, nb_iter=201)
    assert len(xs) == 3 and elapsed > 0
    for k, (case, d, lp, one) in enumerate(zip(cases, golden, lps, singles)):
        xk = one.solve(method="dual_gradient_ascent", get_timing=False, nb_iter=201)
        assert np.array_equal(xs[k], xk), case
        assert lp.itrn_curve == one.itrn_curve == [0, 100, 200]
        for name in ("pobj_curve", "dobj_curve", "max_violated_constraint", "max_violated_equality", "max_violated_inequality",
                     "distance_to_ground_truth", "distanceToGroundTruthAfterRounding", "pobjbound"):
            assert list(getattr(lp, name)) == list(getattr(one, name)), (name, case)
        assert len(lp.opttime_curve) == len(lp.dopttime_curve) == 3
        c, a_eq, b_eq, a_ineq, b_upper, lb, ub = dga_args(d)
        y_eq, y_ineq = lp.dual_multipliers
        n, m_eq, m_in = c.size, a_eq.shape[0], a_ineq.shape[0]
        assert y_eq.shape == (m_eq,) and y_ineq.shape == (m_in,) and isinstance(lp.dual_lower_bound, float)
        # to the bit: the single solver's report at these multipliers
        mat = DeviceMatrix.from_blocks(a_eq, a_ineq, n)
        at = DeviceDGA(mat, np.concatenate((b_eq, b_upper)), c, lb, ub, np.concatenate((y_eq, y_ineq)), m_eq=m_eq)
        try:
            assert lp.dual_lower_bound == at.report()[0], case
        finally:
            at.close()
            mat.close()
        want = dual_energy(c, a_eq, b_eq, a_ineq, b_upper, lb, ub, y_eq, y_ineq)
        c_bar, _ = dual_argmin(c, a_eq, a_ineq, lb, ub, y_eq, y_ineq)
        s_x = np.sum(np.abs(np.minimum(c_bar * ub, c_bar * lb)[c_bar != 0]))
        s_y = np.sum(np.abs(y_eq * b_eq)) + np.sum(np.abs(y_ineq * b_upper))
        bound = 2 * (n + m_eq + m_in + 2) * 2.0 ** -53 * (s_x + s_y)
        print(case, "dual bound", lp.dual_lower_bound, "numpy", want, "difference", abs(lp.dual_lower_bound - want), "allowed", bound)
        assert np.isfinite(want) and abs(lp.dual_lower_bound - want) <= bound, case
        if case == "sc50a":
            # weak duality at the fixture's recorded feasible solution gt, as in the batched suite: D(y) <= c.gt + y.(K gt - b)
            gt = d["gt"]
            assert np.all(gt >= lb) and np.all(gt <= ub)
            slack = y_eq.dot(a_eq * gt - b_eq) + y_ineq.dot(a_ineq * gt - b_upper)
            optimum = c.dot(gt)
            print(case, "dual bound", lp.dual_lower_bound, "c.gt", optimum, "y.(K gt - b)", slack)
            assert lp.dual_lower_bound <= optimum + max(slack, 0.0) + 2 * (n + m_eq + m_in + 2) * 2.0 ** -53 * (abs(optimum) + abs(slack))


def test_gpu_dga_many_raw_abi_refuses_before_any_launch():
    from pysparselp_amd import _lib

    lib = _lib.lib()
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731

    def create(count, n, m_eq, m_in):
        rows = int(sum(m_eq) + sum(m_in))
        cols = int(sum(n))
        indptr = np.arange(rows + 1, dtype=np.int64)
        indices, data = np.zeros(rows, dtype=np.int32), np.ones(rows)
        vec = lambda size: np.zeros(max(size, 1))  # noqa: E731
        return lib.slp_many_dga_create(count, _lib.ptr(i64(*n)), _lib.ptr(i64(*m_eq)), _lib.ptr(i64(*m_in)), _lib.ptr(indptr), _lib.ptr(indices),
                                       _lib.ptr(data), _lib.ptr(vec(rows)), _lib.ptr(vec(cols)), _lib.ptr(vec(cols)), _lib.ptr(vec(cols)),
                                       _lib.ptr(vec(rows)), _lib.ptr(i64(*([0] * len(n)))))

    assert not create(0, [4], [1], [0])
    assert "count must be at least 1" in _lib.last_error()
    assert not create(2, [4, 8193], [1, 1], [0, 1])
    assert "LP 1 has 8193 variables" in _lib.last_error() and "single solver" in _lib.last_error()
    assert not create(2, [4, 5], [0, 1], [0, 2])
    assert "LP 0 needs at least one variable and one constraint row" in _lib.last_error()
    h = create(2, [4, 5], [1, 1], [0, 2])   # a well-formed list is taken
    assert h
    lib.slp_many_dga_destroy(h)
