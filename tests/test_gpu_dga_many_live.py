"""Compaction for dual gradient ascent on a list (csrc/slp_many.h ``k_many_live``, csrc/slp_dga_many.hip ``k_dgm_iterate<., ., true>``:
``DeviceDGAMany.set_compaction`` / ``live_state``, ``dual_gradient_ascent_many_compact``, ``solve_dga_many_compact``) on the GPU.

With compaction on the live LPs -- neither frozen nor stopped -- are handed consecutive workgroups through a list the device builds
in front of every launch.  Which workgroup runs an LP changes none of its bits, so everything here is compared exactly
(``np.array_equal`` or ``==``) and no tolerance appears: with the numpy restatement of tests/dga_many_bound_cases.py, with a state
without compaction driven through the same calls, and the device's list with ``flatnonzero`` of the flags read back.

The references are computed once and shared, never modified.  Needs a real MI355X: run with ``-m gpu``."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse

import dga_many_bound_cases as cases
from dga_batch_cases import batch_case
from dga_many_cases import LP, mixed_list
from test_dga_many_stop_host import ITERATIONS, fifteen
from test_gpu_dga_many import _frozen_list, many_state, snapshot
from test_gpu_dga_many_bound import _assert_full
from test_gpu_dga_many_stop import _assert_iterates, _kmax_env

pytestmark = pytest.mark.gpu

TOL, INF = cases.TOL, np.inf
CALLS = (1, 1, 9, 40, 79)


def _same_snapshot(a, b):
    for p, q in zip(a[:3], b[:3]):   # x, y_eq, y_ineq: lists of per-LP arrays
        assert len(p) == len(q) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(p, q))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5]


def _same_full(a, b):
    assert len(a) == len(b) == 5 and all(np.array_equal(u, v, equal_nan=True) and u.dtype == v.dtype for u, v in zip(a, b))


def _live_of(state):
    """The live LPs by the flags read back: neither stopped nor frozen."""
    return np.flatnonzero(~state.stop_state_full()[1] & ~state.frozen())


def _assert_live_state(state, want, launched=None):
    live, order, got_launched, cap = state.live_state()
    assert order.dtype == np.int32 and live == want.size and np.array_equal(order, want)
    assert launched is None or got_launched == launched
    return cap


# ------------------------------------------------------------------ 1. the fifteen under the cut-off rule, compaction on
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("every", cases.EVERY)
def test_every_lp_stops_where_the_restatement_says_with_compaction_on(monkeypatch, every, kmax):
    _kmax_env(monkeypatch, kmax)
    want = cases.expected([(0, TOL, cases.targets(), every)])
    state = many_state(fifteen())
    try:
        state.set_compaction(True)
        state.set_cutoff(TOL, every, cases.targets())
        state.iterate(ITERATIONS)
        full, snap, report = state.stop_state_full(), snapshot(state), state.report()
        cap = _assert_live_state(state, np.flatnonzero(~want[1]), launched=15)
        assert cap == state.kmax() and (kmax is None or cap == kmax)   # fifteen workgroups or fewer are one round either way
    finally:
        state.close()
    _assert_full(full, want)
    _assert_iterates(snap, want[0])   # a stopped LP has the x of the top of its last iteration, the others ran to the end
    assert want[1].sum() >= 3
    for k in np.flatnonzero(want[1]):
        assert report[k, 0] == full[3][k], k   # the recorded bound is the report's energy, bit for bit


# ------------------------------------------------------------------ 2. on against off, call by call
@pytest.mark.parametrize("kmax", [None, 1])
def test_a_compacted_state_equals_an_uncompacted_one_after_every_call(monkeypatch, kmax):
    _kmax_env(monkeypatch, kmax)
    off, on = many_state(fifteen()), many_state(fifteen())
    try:
        on.set_compaction(True)
        for state in (off, on):
            state.set_cutoff(TOL, 4, cases.targets())
        assert on.live_state()[2:] == (0, 0)   # nothing launched yet
        counts = []
        for k in CALLS:
            before = _live_of(off)
            off.iterate(k)
            on.iterate(k)
            _same_snapshot(snapshot(on), snapshot(off))
            _same_full(on.stop_state_full(), off.stop_state_full())
            assert np.array_equal(on.report(), off.report(), equal_nan=True)
            assert before.size > 0
            _assert_live_state(on, _live_of(off), launched=before.size)   # the grid: the LPs live before the call
            _assert_live_state(off, _live_of(off), launched=15)           # without compaction: the whole list, always
            counts.append(before.size)
        print("live before each call", counts)
        assert counts[0] == 15 and counts[-1] < 15   # the grid did shrink
        _assert_full(on.stop_state_full(), cases.expected([(0, TOL, cases.targets(), 4)]))
    finally:
        off.close()
        on.close()


# ------------------------------------------------------------------ 3. the scan at its edges
@functools.lru_cache(maxsize=None)
def _small_six():
    """The smallest fixture of the mixed list, 48 variables, with each of its six costs; shared, never modified."""
    case = next(case for case, _, args in mixed_list() if args[0].size == 48)
    args, six = batch_case(case)
    assert len(six) == 6
    return tuple((six[cost],) + tuple(args[1:]) for cost in range(6))


def _stages(count):
    """The sets retired stage by stage, cumulative: none; every second LP; also the first half; also a run of 64 across a chunk
    boundary of the scan (where the second half has room for one); all but the last LP; all."""
    ids = np.arange(count)
    per = -(-count // 1024)   # LPs per lane of the scan
    stages = [np.zeros(count, dtype=bool), ids % 2 != (count - 1) % 2]   # every second, of the parity that keeps the last LP
    stages.append(stages[-1] | (ids < count // 2))
    if count - count // 2 > 104:
        edge = per * -(-(count // 2 + 40) // per)   # the first LP of a lane's chunk, inside the second half
        assert edge % per == 0 and count // 2 < edge - 32 and edge + 32 <= count
        stages.append(stages[-1] | ((ids >= edge - 32) & (ids < edge + 32)))
    stages.append(stages[-1] | (ids < count - 1))
    stages.append(np.ones(count, dtype=bool))
    return stages


def _drive(state, count, checked):
    """Retires the LPs of ``state`` stage by stage, one iteration per stage; ``checked``: compare the device's list at every stage."""
    live_before, launched = count, 0
    for retired in _stages(count):
        state.set_cutoff(None, 1, np.where(retired, -1e300, INF))
        state.iterate(1)
        if live_before:
            launched = live_before
        want = np.flatnonzero(~retired)
        if checked:
            assert np.array_equal(_live_of(state), want)   # a cut-off of -1e300 is met at the next check, +inf never
            _assert_live_state(state, want, launched=launched)
        live_before = want.size
    return launched


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_the_device_list_is_the_live_lps_in_increasing_order(count):
    six = _small_six()
    problems = [six[k % 6] for k in range(count)]
    state = many_state(problems)
    try:
        bounds = state.report()[:, 0]
        assert np.all(np.isfinite(bounds)), "the test needs LPs whose bound is finite at every check: a cut-off of -1e300 retires those only"
        assert not state.frozen().any()
        state.set_compaction(True)
        _assert_live_state(state, np.arange(count), launched=0)
        launched = _drive(state, count, checked=True)
        assert launched == 1   # the last launch held the last LP alone
        # everything is retired: a further call launches nothing
        iters = state.status()[3]
        state.iterate(3)
        assert state.status()[3] == iters
        _assert_live_state(state, np.zeros(0, dtype=np.int64), launched=launched)
        if count in (65, 1025):   # ... and the state is that of a list without compaction driven through the same stages
            other = many_state(problems)
            try:
                _drive(other, count, checked=False)
                _same_snapshot(snapshot(state), snapshot(other))
                _same_full(state.stop_state_full(), other.stop_state_full())
                assert other.live_state()[2] == count
            finally:
                other.close()
    finally:
        state.close()


# ------------------------------------------------------------------ 4. frozen LPs, a state that is never armed
def test_a_frozen_lp_is_left_out_of_the_list_of_a_state_that_is_never_armed():
    problems, _ = _frozen_list()
    runs = []
    for compact in (False, True):
        state = many_state(problems)
        try:
            assert state.frozen().tolist() == [False, True, False]
            if compact:
                state.set_compaction(True)
            for k in (1, 9, 40):
                state.iterate(k)
            runs.append((snapshot(state), state.stop_state_full(), state.report()))
            live, order, launched, cap = state.live_state()
            assert live == 2 and order.tolist() == [0, 2] and launched == (2 if compact else 3) and cap == state.kmax()
        finally:
            state.close()
    _same_snapshot(runs[0][0], runs[1][0])
    _same_full(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2], equal_nan=True)
    assert runs[1][1][0].tolist() == [50, 0, 50]


def test_without_a_frozen_lp_an_unarmed_state_launches_the_whole_list():
    runs = []
    for compact in (False, True):
        state = many_state(fifteen())
        try:
            if compact:
                state.set_compaction(True)
            state.iterate(30)
            runs.append(snapshot(state))
            live, order, launched, cap = state.live_state()
            assert live == 15 and order.tolist() == list(range(15)) and launched == 15 and cap == state.kmax()
            state.set_compaction(False)
        finally:
            state.close()
    _same_snapshot(runs[0], runs[1])


# ------------------------------------------------------------------ 5. the new public functions
def _same_info(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=True), key


def _same_lists(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v), (u, v)


@pytest.mark.parametrize("tol, targets", [(TOL, "cut-offs"), (None, "cut-offs"), (1e-2, None)])
def test_dual_gradient_ascent_many_compact_returns_what_the_cutoff_form_returns(tol, targets):
    from pysparselp_amd import dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff

    lps = [LP(*args) for args in fifteen()]
    targets = cases.targets() if targets else None
    old = dual_gradient_ascent_many_cutoff(lps, tol, 10, nb_max_iter=ITERATIONS, targets=targets)
    new = dual_gradient_ascent_many_compact(lps, tol, 10, nb_max_iter=ITERATIONS, targets=targets)
    for a, b in zip(old[:3], new[:3]):
        _same_lists(a, b)
    _same_info(old[3], new[3])
    assert old[3]["stopped"].sum() >= 3


def _sparse_lp(args):
    from pysparselp_amd.SparseLP import SparseLP

    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    if a_ineq is None:   # SparseLP reports its violations from both blocks: an inequality block without rows
        a_ineq, b_upper = scipy.sparse.csr_matrix((0, c.size)), np.zeros(0)
    lp = SparseLP()
    lp.nb_variables = c.size
    lp.costsvector, lp.lower_bounds, lp.upper_bounds = c.copy(), lb.copy(), ub.copy()
    lp.is_integer = np.zeros(c.size, dtype=bool)
    lp.a_equalities, lp.b_equalities = a_eq, b_eq
    lp.a_inequalities, lp.b_lower, lp.b_upper = a_ineq, None, b_upper
    return lp


def test_solve_dga_many_compact_returns_what_the_cutoff_form_returns():
    from pysparselp_amd import solve_dga_many_compact, solve_dga_many_cutoff

    base = [_sparse_lp(args) for args in fifteen()]
    old_lps, new_lps = copy.deepcopy(base), copy.deepcopy(base)
    old = solve_dga_many_cutoff(old_lps, TOL, check_every=10, get_timing=False, nb_iter=ITERATIONS, targets=cases.targets())
    new = solve_dga_many_compact(new_lps, TOL, check_every=10, get_timing=False, nb_iter=ITERATIONS, targets=cases.targets())
    _same_lists(old, new)
    want = cases.expected([(0, TOL, cases.targets(), 10)])
    assert [lp.nb_iterations for lp in new_lps] == want[0].tolist() and [lp.stop_reason for lp in new_lps] == want[4].tolist()
    assert sum(lp.stopped for lp in new_lps) >= 3
    for k, (a, b) in enumerate(zip(old_lps, new_lps)):
        assert (a.nb_iterations, a.stopped, a.stop_reason, a.dual_lower_bound) == (b.nb_iterations, b.stopped, b.stop_reason, b.dual_lower_bound), k
        _same_lists(a.dual_multipliers, b.dual_multipliers)
        assert a.itrn_curve == b.itrn_curve, k


# ------------------------------------------------------------------ 6. the C ABI
def test_the_c_abi_refuses_a_bad_switch_or_handle_and_takes_null_outputs():
    from pysparselp_amd import SlpError, _lib

    state = many_state(fifteen()[:2])
    try:
        lib, h = state._l, state._h
        with pytest.raises(SlpError, match="slp_many_dual_set_compaction: NULL handle"):
            _lib.check(lib.slp_many_dual_set_compaction(None, 1))
        with pytest.raises(SlpError, match="slp_many_dual_live_state: NULL handle"):
            _lib.check(lib.slp_many_dual_live_state(None, None, None, None, None))
        for bad in (2, -1, 7):
            with pytest.raises(SlpError, match="slp_many_dual_set_compaction: on must be 0 or 1"):
                _lib.check(lib.slp_many_dual_set_compaction(h, bad))
        _lib.check(lib.slp_many_dual_live_state(h, None, None, None, None))   # before compaction was ever on: it allocates its list
        live, order, launched, cap = state.live_state()
        assert (live, order.tolist(), launched, cap) == (2, [0, 1], 0, 0)
        for on in (1, 1, 0, 1):
            _lib.check(lib.slp_many_dual_set_compaction(h, on))
        live = np.zeros(1, dtype=np.int64)
        _lib.check(lib.slp_many_dual_live_state(h, _lib.ptr(live), None, None, None))
        assert live[0] == 2
        full = state.stop_state_full()   # no call above changed a record
        assert full[0].tolist() == [0, 0] and not full[1].any() and np.all(full[2] == INF) and np.all(full[3] == -INF)
    finally:
        state.close()
