"""The per-LP stopping test of the Chambolle-Pock list solver (csrc/slp_cp_many.hip: ``CPManyState.set_stop`` / ``stop_state``,
``chambolle_pock_ppd_many_until``, ``solve_many_until``) on the GPU.

The step is a maximum of differences a lane holds, exact in any order, so everything here is compared exactly: the stopping
iteration, the flag and the step (``np.array_equal``) with the numpy restatement (tests/cp_stop_cpu.py on the oracle's iterates),
and every LP's ``x`` and ``y`` with the single solver in SEQUENTIAL order after exactly that LP's number of iterations.  Only the
report's two energies are sums in another fixed order: ``rtol = atol = 1e-9`` as in test_gpu_cp_many.py.

The references (restatement steps, single-solver iterates) are computed once and shared, never modified.  Needs a real MI355X:
run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest

import cp_stop_cpu
from conftest import lp_from_golden, load_golden
from test_cp_many_stop_host import CASES, ITERATIONS, fixture_steps
from test_gpu_cp_many import ENERGY_TOL, ManyRecorder, _advance, _edge_set, _fixture_problem, _mods, _single_walk, form_env  # noqa: F401

pytestmark = pytest.mark.gpu

PIECES = (3, 1, 7, 50, 64, 30)   # uneven iterate calls; the rest in one more
TOL = 1e-2


def _single_state(problem, x0=None):
    CPState, one_sided_system, order = _mods()[2], _mods()[4], _mods()[7]
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    if a_eq is not None and a_eq.shape[0] == 0:
        a_eq, beq = None, None
    ineq, b_ineq = (None, None) if (a_ineq is None or a_ineq.shape[0] == 0) else one_sided_system(a_ineq, bl, bu)
    return CPState(c, a_eq, beq, ineq, b_ineq, lb, ub, x0, 1, 1, order)


def _single_iterates(problem, nb_iter):
    """``([x_0 .. x_T], [y_0 .. y_T])`` of the single solver, one ``iterate(1)`` at a time (read only)."""
    st = _single_state(problem)
    try:
        xs, ys = [st.x()], [st.y()]
        for _ in range(nb_iter):
            st.iterate(1)
            xs.append(st.x())
            ys.append(st.y())
        return xs, ys
    finally:
        st.close()


@functools.lru_cache(maxsize=None)
def _fixture_iterates(case, nb_iter=300):
    """The single solver's iterates of a fixture LP after 0 .. nb_iter iterations."""
    return _single_iterates(_fixture_problem(case), nb_iter)


def _expected(cases, every, total, tol=TOL):
    """``(iterations, stopped, step)`` of the restatement for the fixture LPs."""
    rows = [cp_stop_cpu.stop_state(fixture_steps(c, max(total, ITERATIONS)), tol, every, total) for c in cases]
    return tuple(np.array(col) for col in zip(*rows))


def _make(problems, x0=None):
    CPManyState, prep = _mods()[0], _mods()[5]
    return CPManyState([prep(k, p) for k, p in enumerate(problems)], x0)


def _assert_stop_state(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == np.float64
    print("iterations", got[0], "expected", want[0])
    print("step", got[2], "expected", want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)


def _assert_fixture_iterates(st, cases, iterations):
    xs, ys = st.x(), st.y()
    for k, c in enumerate(cases):
        rx, ry = _fixture_iterates(c)
        assert np.array_equal(xs[k], rx[iterations[k]]), c
        assert np.array_equal(ys[k], ry[iterations[k]]), c


# ------------------------------------------------------------------ 1. stopping iterations and iterates
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("form", [None, "lds", "global"])
@pytest.mark.parametrize("every", [1, 4, 10])
def test_every_lp_stops_where_the_restatement_says(form_env, every, form, kmax):
    form_env(form, kmax)
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        if form is not None:
            assert {st.form(k) for k in range(st.count)} == {form}
        st.set_stop(TOL, every)
        _advance(st, ITERATIONS, PIECES)
        want = _expected(CASES, every, ITERATIONS)
        _assert_stop_state(st.stop_state(), want)
        assert want[0][CASES.index("sc50a")] == ITERATIONS and not want[1][CASES.index("sc50a")] and want[1].sum() == 5
        _assert_fixture_iterates(st, CASES, want[0])
    finally:
        st.close()


def test_the_restatement_on_the_single_solvers_iterates_is_the_one_on_the_oracles():
    """The two sources of iterates the helper is fed from give the same steps."""
    for c in ("sc105", "potts8"):
        xs, ys = _fixture_iterates(c)
        assert np.array_equal(cp_stop_cpu.steps_of(xs[:ITERATIONS + 1], ys[:ITERATIONS + 1]), fixture_steps(c))


# ------------------------------------------------------------------ 2. split iterations
@pytest.mark.parametrize("form", [None, "global"])
@pytest.mark.parametrize("every, stops", [(1, (1, 2, 11, 47, 80)), (4, (1, 2, 11, 48, 80)), (10, (1, 10, 50, 51, 80))])
def test_split_iterations_stop_as_whole_ones(form_env, every, stops, form):
    """``primal_step``, ``report``, ``dual_step`` at stops that include check iterations and the stopping iterations of sc105 and
    potts8: the reduced dx crosses the launch boundary in the control record."""
    form_env(form)
    want = _expected(CASES, every, ITERATIONS)
    assert want[0][CASES.index("sc105")] in stops and want[0][CASES.index("potts8")] in stops
    assert any(s % every == 0 for s in stops)
    singles = [_single_walk(_fixture_problem(c), stops=stops) for c in CASES]
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        st.set_stop(TOL, every)
        done = 0
        for i, s in enumerate(stops):
            _advance(st, s - 1 - done, (3, 1, 7))
            before = st.stop_state()
            st.primal_step()
            rep = st.report()
            st.dual_step()
            done = s
            xs, ys = st.x(), st.y()
            for k, c in enumerate(CASES):
                if before[1][k]:   # stopped before this iteration: no part in it
                    continue
                x, y, r = singles[k][i]
                assert np.array_equal(xs[k], x) and np.array_equal(ys[k], y), (c, s)
                assert np.array_equal(rep[k, 2:5], r[2:5]), (c, s)
                np.testing.assert_allclose(rep[k, :2], r[:2], **ENERGY_TOL)
        _advance(st, ITERATIONS - done, PIECES)
        _assert_stop_state(st.stop_state(), want)
        _assert_fixture_iterates(st, CASES, want[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 3. a stopped LP is not touched
@pytest.mark.parametrize("form", [None, "global"])
def test_a_stopped_lp_is_not_touched(form_env, form):
    form_env(form)
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        st.set_stop(TOL, 1)
        _advance(st, ITERATIONS, PIECES)
        st.primal_step()   # a reporting iteration, so that x4 of the running LP is current
        rep0 = st.report()
        st.dual_step()
        x0, y0, state0 = st.x(), st.y(), st.stop_state()
        stopped = state0[1]
        assert list(stopped) == [c != "sc50a" for c in CASES]
        st.iterate(5)
        st.primal_step()
        rep1 = st.report()
        st.dual_step()
        st.primal_step()
        st.dual_step()
        st.iterate(3)
        x1, y1, state1 = st.x(), st.y(), st.stop_state()
        total = ITERATIONS + 1 + 5 + 1 + 1 + 3
        for k, c in enumerate(CASES):
            if stopped[k]:
                assert np.array_equal(x1[k], x0[k]) and np.array_equal(y1[k], y0[k]), c
                assert np.array_equal(rep1[k], rep0[k]), c   # x, x4, z, y all as they were
                assert all(np.array_equal(a[k], b[k]) for a, b in zip(state0, state1)), c
            else:
                assert state1[0][k] == total and not state1[1][k]
        _assert_fixture_iterates(st, CASES, state1[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 4. off is today
@pytest.mark.parametrize("form", [None, "lds", "global"])
@pytest.mark.parametrize("armed_first", [False, True])
def test_without_the_test_every_lp_runs_all_iterations(form_env, armed_first, form):
    form_env(form)
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        if armed_first:
            st.set_stop(TOL, 1)
            st.set_stop(None)
        _advance(st, ITERATIONS, PIECES)
        n = len(CASES)
        _assert_stop_state(st.stop_state(), (np.full(n, ITERATIONS), np.zeros(n, dtype=bool), np.full(n, np.inf)))
        _assert_fixture_iterates(st, CASES, [ITERATIONS] * n)
    finally:
        st.close()


def test_the_c_abi_refuses_a_bad_tolerance_or_cadence(form_env):
    from pysparselp_amd import SlpError, _lib

    st = _make([_fixture_problem("random0")])
    try:
        for tol, every in ((float("nan"), 1), (float("inf"), 1), (1e-2, 0), (0.0, -1)):
            with pytest.raises(SlpError, match="slp_many_cp_set_stop"):
                _lib.check(st._l.slp_many_cp_set_stop(st._h, tol, every))
        _lib.check(st._l.slp_many_cp_set_stop(st._h, -1.0, 0))   # off: the cadence is not looked at
        _lib.check(st._l.slp_many_cp_stop_state(st._h, None, None, None))
    finally:
        st.close()


# ------------------------------------------------------------------ 5. re-arming
def test_a_new_tolerance_lets_the_stopped_lps_go_on(form_env):
    first, more = 100, 200
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        st.set_stop(TOL, 1)
        _advance(st, first, PIECES)
        state = st.stop_state()
        _assert_stop_state(state, _expected(CASES, 1, first))
        assert state[1].sum() == 5
        st.set_stop(1e-3, 1)
        cleared = st.stop_state()
        assert not cleared[1].any() and np.array_equal(cleared[0], state[0]) and np.array_equal(cleared[2], state[2])
        _advance(st, more, PIECES)
        rows = []
        for k, c in enumerate(CASES):
            t0 = int(state[0][k])
            rows.append(cp_stop_cpu.stop_state(fixture_steps(c, 300), 1e-3, 1, t0 + more, after=t0, step_before=state[2][k]))
        want = tuple(np.array(col) for col in zip(*rows))
        got = st.stop_state()
        _assert_stop_state(got, want)
        by_case = dict(zip(CASES, zip(*got)))
        assert all(by_case[c][1] for c in ("potts8", "random0", "random1", "random2"))
        assert not by_case["sc105"][1] and not by_case["sc50a"][1] and by_case["sc50a"][0] == first + more
        _assert_fixture_iterates(st, CASES, got[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 6. an exact fixed point
@pytest.mark.parametrize("form", [None, "global"])
def test_tolerance_zero_stops_at_a_fixed_point(form_env, form):
    form_env(form)
    st = _make([_fixture_problem("potts8")])
    try:
        st.set_stop(0.0, 1)
        _advance(st, ITERATIONS, PIECES)
        want = _expected(["potts8"], 1, ITERATIONS, tol=0.0)
        assert want[1][0] and want[2][0] == 0.0
        got = st.stop_state()
        _assert_stop_state(got, want)
        assert got[2][0] == 0.0
        _assert_fixture_iterates(st, ["potts8"], want[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 7. shapes where lanes loop
def test_lanes_that_loop_and_single_kinds_of_rows(form_env):
    """potts50 (7400 variables on 1024 lanes, the global form by its size), an LP with equality rows only and one with a single
    row; the last two cannot go through the oracle: their iterates are the single solver's, one iteration at a time."""
    total = 130
    edge = dict(_edge_set())
    problems = [_fixture_problem("potts50"), edge["equalities_only"], edge["one_row"]]
    steps = [cp_stop_cpu.steps_of(*cp_stop_cpu.oracle_iterates(problems[0], total))]
    iterates = [_single_iterates(p, total) for p in problems]
    steps += [cp_stop_cpu.steps_of(*it) for it in iterates[1:]]
    assert np.array_equal(cp_stop_cpu.steps_of(*iterates[0]), steps[0])
    want = tuple(np.array(col) for col in zip(*[cp_stop_cpu.stop_state(s, TOL, 1, total) for s in steps]))
    assert want[1][0] and 1 < want[0][0] < total
    st = _make(problems)
    try:
        assert [st.form(k) for k in range(3)] == ["global", "lds", "lds"]
        st.set_stop(TOL, 1)
        _advance(st, total, PIECES)
        _assert_stop_state(st.stop_state(), want)
        xs, ys = st.x(), st.y()
        for k in range(3):
            assert np.array_equal(xs[k], iterates[k][0][want[0][k]]) and np.array_equal(ys[k], iterates[k][1][want[0][k]]), k
    finally:
        st.close()


# ------------------------------------------------------------------ 8. a NaN in the data
@pytest.mark.parametrize("form", [None, "global"])
def test_an_lp_with_a_nan_never_stops_and_leaves_the_others_alone(form_env, form):
    form_env(form)
    total = 100
    c, *rest = _fixture_problem("random0")
    c = np.array(c, copy=True)
    c[3] = np.nan
    bad = (c, *rest)
    iterates = _single_iterates(bad, total)
    row = cp_stop_cpu.stop_state(cp_stop_cpu.steps_of(*iterates), TOL, 1, total)
    assert row[0] == total and not row[1] and np.isnan(row[2])
    others = _expected(["potts8", "sc105"], 1, total)
    assert others[1].all()
    want = tuple(np.concatenate(([a], b)) for a, b in zip(row, others))
    st = _make([bad, _fixture_problem("potts8"), _fixture_problem("sc105")])
    try:
        st.set_stop(TOL, 1)
        _advance(st, total, PIECES)
        got = st.stop_state()
        _assert_stop_state(got, want)
        xs, ys = st.x(), st.y()
        assert np.array_equal(xs[0], iterates[0][total], equal_nan=True) and np.array_equal(ys[0], iterates[1][total], equal_nan=True)
        assert np.isnan(xs[0]).any()
        for k, case in ((1, "potts8"), (2, "sc105")):
            rx, ry = _fixture_iterates(case)
            assert np.array_equal(xs[k], rx[got[0][k]]) and np.array_equal(ys[k], ry[got[0][k]])
    finally:
        st.close()


# ------------------------------------------------------------------ 9. the drivers
class InfoRecorder(ManyRecorder):
    """Also keeps the ``info`` the driver sets as an attribute of its callback, as it is at every call."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __call__(self, *report):
        super().__call__(*report)
        self.seen.append({name: values.copy() for name, values in self.info.items()})


@pytest.mark.parametrize("with_sc50a, every", [(False, 1), (True, 10)])
def test_the_list_driver_ends_when_every_lp_has_stopped(form_env, with_sc50a, every):
    from pysparselp_amd import chambolle_pock_ppd_many_until

    cases = [c for c in CASES if with_sc50a or c != "sc50a"]
    want = _expected(cases, every, ITERATIONS)
    rec = InfoRecorder()
    xs, best, info = chambolle_pock_ppd_many_until([_fixture_problem(c) for c in cases], TOL, every, nb_max_iter=ITERATIONS,
                                                   callback_func=rec, nb_iter_plot=10)
    _assert_stop_state((info["iterations"], info["stopped"], info["step"]), want)
    assert len(best) == len(cases)
    if with_sc50a:
        assert rec.it == list(range(0, ITERATIONS, 10)) and info["iterations"][cases.index("sc50a")] == ITERATIONS
    else:   # the first report index at which every LP is stopped gets no callback
        last = int(want[0].max())
        assert last < ITERATIONS - 10 and rec.it == list(range(0, last, 10))
    for k, c in enumerate(cases):
        rx, _ = _fixture_iterates(c)
        assert np.array_equal(xs[k], rx[want[0][k]]), c
        rows = np.array([[store[i][k] for store in (rec.e1, rec.e2, rec.veq, rec.vineq)] for i in range(len(rec.it))])
        for i, niter in enumerate(rec.it):
            is_stopped = bool(want[1][k]) and want[0][k] <= niter
            assert rec.seen[i]["stopped"][k] == is_stopped, (c, niter)
            if is_stopped:   # its final iterate, and the last row it had while it was running
                assert rec.seen[i]["iterations"][k] == want[0][k]
                assert np.array_equal(rec.x[i][k], xs[k]) and np.array_equal(rows[i], rows[i - 1]), (c, niter)
            else:
                assert rec.seen[i]["iterations"][k] == niter


def _golden_lps():
    from pysparselp_amd.SparseLP import SparseLP

    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("sc50a", "potts8", "random1", "sc105", "random0")]
    lp = lps[2]   # a tenth of its variables fixed through equal bounds
    fixed = np.arange(0, lp.nb_variables, 10)
    value = np.clip(0.25, lp.lower_bounds[fixed], lp.upper_bounds[fixed])
    lp.lower_bounds[fixed] = value
    lp.upper_bounds[fixed] = value
    return lps


@pytest.mark.parametrize("every", [10, 1])
def test_solve_many_until_equals_solve_for_each_lps_own_count(form_env, every):
    from pysparselp_amd import ORDER_SEQUENTIAL, solve_many_until

    lps, singles = _golden_lps(), _golden_lps()
    xs, elapsed = solve_many_until(lps, TOL, check_every=every, nb_iter=ITERATIONS, nb_iter_plot=10)
    assert elapsed > 0 and len(xs) == len(lps)
    print("iterations", [lp.nb_iterations for lp in lps], "stopped", [lp.stopped for lp in lps])
    assert not lps[0].stopped and lps[0].nb_iterations == ITERATIONS
    assert lps[1].stopped and lps[3].stopped and lps[4].stopped
    assert len({lp.nb_iterations for lp in lps}) >= 3
    for k, lp in enumerate(singles):
        got = lps[k]
        assert (got.nb_iterations < ITERATIONS) == got.stopped and (not got.stopped or got.nb_iterations % every == 0)
        x, _ = lp.solve(method="chambolle_pock_ppd", nb_iter=got.nb_iterations, nb_iter_plot=10, order=ORDER_SEQUENTIAL, setup="host")
        assert x.shape == (lp.nb_variables,) and np.array_equal(xs[k], x), k
        assert got.itrn_curve == lp.itrn_curve == list(range(0, got.nb_iterations, 10))
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.asarray(getattr(got, name), dtype=np.float64), np.asarray(getattr(lp, name), dtype=np.float64)), (k, name)
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(getattr(got, name), getattr(lp, name), **ENERGY_TOL)
        assert len(got.opttime_curve) == len(got.dopttime_curve) == len(got.itrn_curve)
