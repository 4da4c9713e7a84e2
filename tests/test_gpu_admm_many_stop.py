"""The per-LP stopping test of the ADMM list solver (csrc/slp_admm_many.hip: ``ADMMManyState.set_stop`` / ``stop_state``,
``lp_admm_many_until``, ``solve_admm_many_until``) on the GPU.

The residual and the step are maxima of values a lane holds, exact in any order, so everything here is compared exactly: the
stopping iteration, the flag, the residual and the step (``np.array_equal``) with the numpy restatement (tests/admm_stop_cpu.py on
the oracle's iterates), and every LP's ``x`` (all ``N`` columns) and ``lambda`` with the single solver in SEQUENTIAL order after
exactly that LP's number of iterations.  Only the report's energy is a sum in another fixed order: ``rtol = atol = 1e-9`` as in
test_gpu_admm_many.py.

The references (restatement curves, single-solver iterates) are computed once and shared, never modified.  Needs a real MI355X:
run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest
import scipy.sparse

import admm_stop_cpu
from conftest import lp_from_golden, load_golden
from test_admm_many_stop_host import CASES, ITERATIONS, fixture_curves
from test_gpu_admm_many import ENERGY_TOL, ListRecorder, _many_state, _mods, _problem

pytestmark = pytest.mark.gpu

PIECES = (3, 1, 7, 50, 64, 30)   # uneven iterate calls; the rest in one more
TOL = (1e-3, 1e-3)               # three of the six LPs stop, at distinct iterations (test_admm_many_stop_host.py)
LOOSE = (1e-2, 1e-2)             # all six stop


@pytest.fixture()
def form_env(monkeypatch):
    """Sets the two switches the library reads when a list is created."""
    def use(form=None, kmax=None):
        for name, v in (("SLP_ADMM_MANY_FORM", form), ("SLP_ADMM_MANY_KMAX", kmax)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))

    use()
    yield use
    use()


def _advance(st, k, pieces=PIECES):
    for step in pieces:
        if k >= step:
            st.iterate(step)
            k -= step
    st.iterate(k)


def _single_state(problem):
    ADMMState, seq = _mods()[2], _mods()[4]
    return ADMMState.from_lp(*problem, None, 2, 3, True, order=seq)


def _single_iterates(problem, nb_iter):
    """``([x_0 .. x_T] over all N, [lambda_0 .. lambda_T], [residual_1 .. residual_T])`` of the single solver, one ``iterate(1)`` at
    a time; the residual is column 1 of its report (read only)."""
    st = _single_state(problem)
    try:
        xs, lams, residuals = [st.x()], [st.lam()], []
        for _ in range(nb_iter):
            st.iterate(1)
            xs.append(st.x())
            lams.append(st.lam())
            residuals.append(float(st.report()[1]))
        return xs, lams, residuals
    finally:
        st.close()


def _single_at(problem, t):
    """``(x over all N, lambda)`` of the single solver after ``t`` iterations."""
    st = _single_state(problem)
    try:
        st.iterate(int(t))
        return st.x(), st.lam()
    finally:
        st.close()


@functools.lru_cache(maxsize=None)
def _fixture_iterates(case):
    """The single solver's iterates of a fixture LP after 0 .. ITERATIONS iterations."""
    return _single_iterates(_problem(case), ITERATIONS)


@functools.lru_cache(maxsize=None)
def _single_split(case, stops):
    """The single solver at every stop ``s``: after ``s - 1`` iterations and the sweep of the next: (x, lambda, report)."""
    st = _single_state(_problem(case))
    try:
        out, done = [], 0
        for s in stops:
            st.iterate(s - 1 - done)
            st.sweep_step()
            out.append((st.x(), st.lam(), st.report()[:3].copy()))
            st.multiplier_step()
            done = s
        return out
    finally:
        st.close()


def _columns(rows):
    return tuple(np.array(col) for col in zip(*rows))


def _expected(cases, tols, every, total):
    """``(iterations, stopped, residual, step)`` of the restatement for the fixture LPs."""
    return _columns([admm_stop_cpu.stop_state(*fixture_curves(c), *tols, every, total) for c in cases])


def _assert_stop_state(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == np.float64 and got[3].dtype == np.float64
    print("iterations", got[0], "expected", want[0])
    print("residual", got[2], "expected", want[2])
    print("step", got[3], "expected", want[3])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)
    assert np.array_equal(got[3], want[3], equal_nan=True)


def _assert_fixture_iterates(st, cases, iterations):
    xs, lams = st.x(full=True), st.lam()
    for k, c in enumerate(cases):
        rx, rl, _ = _fixture_iterates(c)
        assert np.array_equal(xs[k], rx[iterations[k]]), c
        assert np.array_equal(lams[k], rl[iterations[k]]), c


# ------------------------------------------------------------------ 1. stopping iterations and iterates
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("form", [None, "lds", "global"])
@pytest.mark.parametrize("every", [1, 4, 10])
def test_every_lp_stops_where_the_restatement_says(form_env, every, form, kmax):
    form_env(form, kmax)
    st = _many_state([_problem(c) for c in CASES])
    try:
        if form is not None:
            assert {st.form(k) for k in range(st.count)} == {form}
        if kmax is not None:
            assert st.kmax(form or "lds") == kmax
        st.set_stop(*TOL, every)
        _advance(st, ITERATIONS)
        want = _expected(CASES, TOL, every, ITERATIONS)
        assert want[1].sum() == 3 and len(set(want[0][want[1]])) == 3 and (want[0][~want[1]] == ITERATIONS).all()
        got = st.stop_state()
        _assert_stop_state(got, want)
        _assert_fixture_iterates(st, CASES, want[0])
        # a stopped LP is frozen at its test, a running one was tested at the last iteration: the report's residual is the test's
        assert ITERATIONS % every == 0 and np.array_equal(st.report()[:, 1], got[2])
    finally:
        st.close()


# ------------------------------------------------------------------ 2. the two sources of curves
def test_the_restatement_on_the_single_solvers_iterates_is_the_one_on_the_oracles():
    for c in CASES:
        xs, _, residuals = _fixture_iterates(c)
        residual, step = admm_stop_cpu.curves_of(xs, residuals)
        assert np.array_equal(residual, fixture_curves(c)[0]), c
        assert np.array_equal(step, fixture_curves(c)[1]), c


# ------------------------------------------------------------------ 3. split iterations
@pytest.mark.parametrize("form", [None, "global"])
@pytest.mark.parametrize("every, stops", [(1, (1, 2, 11, 140, 178)), (4, (1, 2, 12, 140, 180)), (10, (1, 10, 51, 140, 180))])
def test_split_iterations_stop_as_whole_ones(form_env, every, stops, form):
    """``sweep_step``, ``report``, ``multiplier_step`` at stops that include check iterations and the stopping iterations of potts8
    and random1: the reduced step crosses the launch boundary in the control record."""
    form_env(form)
    want = _expected(CASES, TOL, every, ITERATIONS)
    assert want[0][CASES.index("potts8")] in stops and want[0][CASES.index("random1")] in stops
    assert any(s % every == 0 for s in stops) and (every == 1 or any(s % every for s in stops))
    st = _many_state([_problem(c) for c in CASES])
    try:
        st.set_stop(*TOL, every)
        done = 0
        for i, s in enumerate(stops):
            _advance(st, s - 1 - done, (3, 1, 7))
            before = st.stop_state()
            st.sweep_step()
            rep = st.report()
            xs, lams = st.x(full=True), st.lam()
            st.multiplier_step()
            done = s
            for k, c in enumerate(CASES):
                if before[1][k]:   # stopped before this iteration: no part in it
                    continue
                x, lam, r = _single_split(c, stops)[i]
                assert np.array_equal(xs[k], x) and np.array_equal(lams[k], lam), (c, s)
                assert np.array_equal(rep[k, 1:], r[1:]), (c, s)
                np.testing.assert_allclose(rep[k, 0], r[0], **ENERGY_TOL)
        _advance(st, ITERATIONS - done)
        _assert_stop_state(st.stop_state(), want)
        _assert_fixture_iterates(st, CASES, want[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 4. sixteen waves beside one
def _tiny_problem():
    """One variable, one inequality row."""
    return (np.array([1.0]), None, None, scipy.sparse.csr_matrix(np.array([[2.0]])), np.array([0.5]), np.array([1.5]), np.array([0.0]),
            np.array([1.0]))


def test_potts50_on_sixteen_waves_beside_a_tiny_lp(form_env):
    """potts50 is in the global form by its size (2 N + m = 44 200 doubles) on a workgroup of 1024 lanes: the fold runs over all
    sixteen wave slots, and most lanes have no row in most levels.  The tiny LP is the smallest workgroup, one lane with a row."""
    total = 140
    problems = [_problem("potts50"), _tiny_problem()]
    curves = [admm_stop_cpu.oracle_curves(p, total) for p in problems]
    want = _columns([admm_stop_cpu.stop_state(*c, *LOOSE, 10, total) for c in curves])
    assert want[1].all() and want[0][0] == 130 and 1 < want[0][1] < 130
    st = _many_state(problems)
    try:
        assert [st.form(k) for k in range(2)] == ["global", "lds"]
        st.set_stop(*LOOSE, 10)
        _advance(st, total)
        got = st.stop_state()
        _assert_stop_state(got, want)
        xs, lams, rep = st.x(full=True), st.lam(), st.report()
        for k, p in enumerate(problems):
            x, lam = _single_at(p, want[0][k])
            assert np.array_equal(xs[k], x) and np.array_equal(lams[k], lam), k
        assert np.array_equal(rep[:, 1], got[2])
    finally:
        st.close()


# ------------------------------------------------------------------ 5. re-arming
def test_a_new_call_clears_the_flags_and_keeps_the_counters(form_env):
    first, more = 100, 100
    st = _many_state([_problem(c) for c in CASES])
    try:
        st.set_stop(*LOOSE, 1)
        _advance(st, first)
        state = st.stop_state()
        _assert_stop_state(state, _expected(CASES, LOOSE, 1, first))
        assert state[1].sum() == 4
        st.set_stop(*TOL, 1)
        cleared = st.stop_state()
        assert not cleared[1].any() and all(np.array_equal(cleared[j], state[j]) for j in (0, 2, 3))
        _advance(st, more)
        rows = []
        for k, c in enumerate(CASES):
            t0 = int(state[0][k])
            assert t0 + more <= ITERATIONS
            rows.append(admm_stop_cpu.stop_state(*fixture_curves(c), *TOL, 1, t0 + more, after=t0, before=(state[2][k], state[3][k])))
        got = st.stop_state()
        _assert_stop_state(got, _columns(rows))
        assert got[1][CASES.index("potts8")] and not got[1][CASES.index("sc50a")]
        _assert_fixture_iterates(st, CASES, got[0])
    finally:
        st.close()


@pytest.mark.parametrize("form", [None, "global"])
def test_armed_with_tolerance_zero_is_the_unarmed_run(form_env, form):
    form_env(form)
    total = 50
    states = [_many_state([_problem(c) for c in CASES]) for _ in range(2)]
    try:
        states[0].set_stop(0.0, 0.0, 1)
        for st in states:
            _advance(st, total, (3, 1, 7))
        n = len(CASES)
        armed, off = states[0].stop_state(), states[1].stop_state()
        _assert_stop_state(armed, _expected(CASES, (0.0, 0.0), 1, total))
        _assert_stop_state(off, (np.full(n, total), np.zeros(n, dtype=bool), np.full(n, np.inf), np.full(n, np.inf)))
        assert not armed[1].any() and np.array_equal(armed[0], off[0])
        for a, b in zip(states[0].x(full=True) + states[0].lam(), states[1].x(full=True) + states[1].lam()):
            assert np.array_equal(a, b)
        _assert_fixture_iterates(states[0], CASES, [total] * n)
    finally:
        for st in states:
            st.close()


def test_the_iterations_run_while_the_test_is_off_are_counted(form_env):
    """Armed for 30 iterations, off for 25, armed again: the cadence goes by the count of the LP's life (the next test is at
    iteration 60), and the values of the last test are kept while the test is off."""
    st = _many_state([_problem(c) for c in CASES])
    try:
        st.set_stop(*TOL, 10)
        _advance(st, 30, (3, 1, 7))
        armed = st.stop_state()
        _assert_stop_state(armed, _expected(CASES, TOL, 10, 30))
        st.set_stop(None, None)
        _advance(st, 25, (3, 1, 7))
        off = st.stop_state()
        assert np.array_equal(off[0], np.full(len(CASES), 55)) and not off[1].any()
        assert np.array_equal(off[2], armed[2]) and np.array_equal(off[3], armed[3])
        st.set_stop(*TOL, 10)
        assert np.array_equal(st.stop_state()[0], off[0])
        _advance(st, ITERATIONS - 55)
        rows = [admm_stop_cpu.stop_state(*fixture_curves(c), *TOL, 10, ITERATIONS, after=55, before=(armed[2][k], armed[3][k]))
                for k, c in enumerate(CASES)]
        want = _columns(rows)
        assert np.array_equal(want[0], _expected(CASES, TOL, 10, ITERATIONS)[0])   # no LP of the list stops before iteration 60
        got = st.stop_state()
        _assert_stop_state(got, want)
        _assert_fixture_iterates(st, CASES, got[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 6. the C entry
def test_the_c_abi_refuses_bad_arguments_and_a_call_inside_an_iteration(form_env):
    from pysparselp_amd import SlpError, _lib

    st = _many_state([_problem("random0")])
    try:
        set_stop, nan, inf = st._l.slp_many_admm_set_stop, float("nan"), float("inf")
        for args in ((nan, 0.0, 1), (inf, 0.0, 1), (0.0, nan, 1), (0.0, inf, 1), (0.0, -1.0, 1), (1e-2, 1e-2, 0), (0.0, 0.0, -1)):
            with pytest.raises(SlpError, match="slp_many_admm_set_stop"):
                _lib.check(set_stop(st._h, *args))
        _lib.check(set_stop(st._h, -1.0, nan, 0))   # off: the step tolerance and the cadence are not looked at
        _lib.check(st._l.slp_many_admm_stop_state(st._h, None, None, None, None))
        st.sweep_step()
        for args in ((1e-2, 1e-2, 1), (-1.0, 0.0, 1)):
            with pytest.raises(SlpError, match="slp_many_admm_set_stop.*between sweep_step and multiplier_step"):
                _lib.check(set_stop(st._h, *args))
        with pytest.raises(SlpError, match="slp_many_admm_set_stop"):
            st.set_stop(1e-2, 1e-2)
        st.multiplier_step()
        st.set_stop(1e-2, 1e-2)
        iterations, stopped, residual, step = st.stop_state()
        assert iterations[0] == 1 and not stopped[0] and residual[0] == np.inf and step[0] == np.inf
    finally:
        st.close()


# ------------------------------------------------------------------ 7. the drivers
class InfoRecorder(ListRecorder):
    """Every report, and the ``info`` the driver sets as an attribute of its callback, as it is at every call."""

    def __init__(self):
        super().__init__(range(ITERATIONS + 1))
        self.seen = []

    def __call__(self, *report):
        super().__call__(*report)
        self.seen.append({name: values.copy() for name, values in self.info.items()})


@pytest.mark.parametrize("tols, every", [(TOL, 10), (LOOSE, 1)])
def test_the_list_driver_ends_when_every_lp_has_stopped(form_env, tols, every):
    from pysparselp_amd import lp_admm_many_until

    want = _expected(CASES, tols, every, ITERATIONS)
    rec = InfoRecorder()
    xs, info = lp_admm_many_until([_problem(c) for c in CASES], *tols, every, nb_iter=ITERATIONS - 1, callback_func=rec, nb_iter_plot=10)
    assert info is rec.info and sorted(info) == ["iterations", "residual", "step", "stopped"]
    _assert_stop_state((info["iterations"], info["stopped"], info["residual"], info["step"]), want)
    if want[1].all():   # the first report index at which every LP is stopped gets no callback
        last = int(want[0].max())
        assert last < ITERATIONS - 10 and rec.it == list(range(0, last, 10))
    else:
        assert rec.it == list(range(0, ITERATIONS, 10))
    for k, c in enumerate(CASES):
        n = _problem(c)[0].size
        rx = _fixture_iterates(c)[0]
        assert np.array_equal(xs[k], rx[want[0][k]][:n]), c
        for i, niter in enumerate(rec.it):
            is_stopped = bool(want[1][k]) and want[0][k] <= niter
            assert rec.seen[i]["stopped"][k] == is_stopped, (c, niter)
            if is_stopped:   # its final iterate, and the report of the frozen state
                assert rec.seen[i]["iterations"][k] == want[0][k]
                assert np.array_equal(rec.x[i][k], xs[k]), (c, niter)
                assert rec.veq[i][k] == info["residual"][k] == want[2][k], (c, niter)
                assert rec.vineq[i][k] == max(0.0, -rx[want[0][k]].min()), (c, niter)
            else:
                assert rec.seen[i]["iterations"][k] == niter
                if niter in (0, 10):   # a running LP's xs[k] is the iterate of the report: one sweep ahead of its count
                    assert np.array_equal(rec.x[i][k], _single_report_x(c, niter)[:n]), (c, niter)


@functools.lru_cache(maxsize=None)
def _single_report_x(case, niter):
    """x of the single solver at report index ``niter``: after ``niter`` iterations and one more sweep."""
    return _single_split(case, (niter + 1,))[0][0]


def test_max_time_ends_the_list_at_the_first_report(form_env):
    from pysparselp_amd import lp_admm_many_until

    rec = InfoRecorder()
    xs, info = lp_admm_many_until([_problem(c) for c in ("random0", "potts8")], *LOOSE, 1, nb_iter=ITERATIONS, callback_func=rec, max_time=0.0)
    assert rec.it == [] and len(xs) == 2
    assert np.array_equal(info["iterations"], [0, 0]) and not info["stopped"].any()
    assert np.array_equal(info["residual"], [np.inf, np.inf]) and np.array_equal(info["step"], [np.inf, np.inf])


def _golden_lps():
    from pysparselp_amd.SparseLP import SparseLP

    return [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in CASES]


@pytest.mark.parametrize("tols, every", [(TOL, 10), (LOOSE, 1)])
def test_solve_admm_many_until_equals_solve_for_each_lps_own_count(form_env, tols, every):
    from pysparselp_amd import ORDER_SEQUENTIAL, solve_admm_many_until

    want = _expected(CASES, tols, every, ITERATIONS)
    lps, singles = _golden_lps(), _golden_lps()
    xs, elapsed = solve_admm_many_until(lps, *tols, check_every=every, nb_iter=ITERATIONS - 1, nb_iter_plot=10)
    assert elapsed > 0 and len(xs) == len(lps)
    print("iterations", [lp.nb_iterations for lp in lps], "stopped", [lp.stopped for lp in lps])
    assert [lp.nb_iterations for lp in lps] == list(want[0]) and [lp.stopped for lp in lps] == list(want[1])
    for k, lp in enumerate(singles):
        got = lps[k]
        x, _ = lp.solve(method="admm", nb_iter=got.nb_iterations - 1, nb_iter_plot=10, order=ORDER_SEQUENTIAL, setup="host")
        assert x.shape == (lp.nb_variables,) and np.array_equal(xs[k], x), k
        assert got.itrn_curve == lp.itrn_curve == list(range(0, got.nb_iterations, 10))
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.asarray(getattr(got, name), dtype=np.float64), np.asarray(getattr(lp, name), dtype=np.float64)), (k, name)
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(getattr(got, name), getattr(lp, name), **ENERGY_TOL)
        assert len(got.opttime_curve) == len(got.dopttime_curve) == len(got.itrn_curve)
