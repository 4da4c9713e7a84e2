"""The certificate as the per-LP stopping test of the Chambolle-Pock list solver (csrc/slp_cp_many.hip: ``CPManyState.set_stop_gap``
/ ``gap_state``, ``chambolle_pock_ppd_many_certified``, ``solve_many_certified``) on the GPU.

The violation is a maximum over single-accumulator chains in storage order: compared exactly with the numpy restatement
(tests/cp_gap_cpu.py).  ``primal`` and ``lower_bound`` are sums in the kernel's fixed order against numpy's: ``rtol = atol = 1e-9``,
the suite's bar for sums in another fixed order.  The stopping iteration and the flag are compared exactly (``np.array_equal``) for
every LP all of whose checks are decidable -- more than 1000 bands of rounding from their threshold, which
tests/test_cp_many_gap_host.py asserts for the lists used here on the restatement alone -- and every LP's ``x`` and ``y`` are bit
for bit the single solver's (or the oracle's) after exactly that LP's number of iterations.

The references are computed once and shared, never modified.  Needs a real MI355X: run with ``-m gpu``.
"""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse

import cp_gap_cpu
from test_cp_many_gap_host import (RANDOM_EVERY, RANDOM_ITERATIONS, TOL_FEAS, TOL_GAP, fixture_certificates, random_certificates,
                                   random_left_out, random_problems)
from test_cp_many_stop_host import CASES, ITERATIONS
from test_gpu_cp_many import ENERGY_TOL, _advance, _fixture_problem, form_env  # noqa: F401
from test_gpu_cp_many_stop import PIECES, InfoRecorder, _fixture_iterates, _golden_lps, _make

pytestmark = pytest.mark.gpu

NAMES = ("iterations", "stopped", "primal", "lower_bound", "violation")


def _expected(certs, every, total, tol=(TOL_GAP, TOL_FEAS)):
    """The columns of ``gap_state`` from the restatement."""
    rows = [cp_gap_cpu.gap_state(cert, tol[0], tol[1], every, total) for cert in certs]
    return tuple(np.array(col) for col in zip(*rows))


def _assert_gap_state(got, want, keep=None):
    """``keep``: the LPs whose stopping iteration is compared (all when None); the others' records are compared where both sides
    evaluated the same check last."""
    assert got[0].dtype == np.int64 and got[1].dtype == bool and all(v.dtype == np.float64 for v in got[2:])
    for name, g, w in zip(NAMES, got, want):
        print(name, g, "expected", w)
    keep = np.ones(len(got[0]), dtype=bool) if keep is None else keep
    assert np.array_equal(got[0][keep], want[0][keep])
    assert np.array_equal(got[1][keep], want[1][keep])
    same = keep | (got[0] == want[0])
    assert np.array_equal(got[4][same], want[4][same], equal_nan=True)
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(got[2][same], want[2][same], **ENERGY_TOL)
        np.testing.assert_allclose(got[3][same], want[3][same], **ENERGY_TOL)


def _assert_fixture_iterates(st, cases, iterations):
    xs, ys = st.x(), st.y()
    for k, c in enumerate(cases):
        rx, ry = _fixture_iterates(c)
        assert np.array_equal(xs[k], rx[iterations[k]]), c
        assert np.array_equal(ys[k], ry[iterations[k]]), c


def _host_decision(primal, bound, violation, tol_gap, tol_feas):
    return cp_gap_cpu.decision(primal, bound, violation, tol_gap, tol_feas)


# ------------------------------------------------------------------ 1. stopping iterations, records and iterates
@pytest.mark.parametrize("kmax", [None, 1, 7])
@pytest.mark.parametrize("form", [None, "lds", "global"])
@pytest.mark.parametrize("every", [1, 4, 10])
def test_every_lp_stops_where_the_restatement_says(form_env, every, form, kmax):  # noqa: F811
    form_env(form, kmax)
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        if form is not None:
            assert {st.form(k) for k in range(st.count)} == {form}
        st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        _advance(st, ITERATIONS, PIECES)
        want = _expected([fixture_certificates(c) for c in CASES], every, ITERATIONS)
        got = st.gap_state()
        _assert_gap_state(got, want)
        assert want[1].sum() == 4 and not want[1][CASES.index("sc50a")] and not want[1][CASES.index("sc105")]
        assert np.array_equal(st.stop_state()[0], got[0]) and np.array_equal(st.stop_state()[1], got[1])
        _assert_fixture_iterates(st, CASES, want[0])
    finally:
        st.close()


# ------------------------------------------------------------------ 2. the device's decision is the one its own numbers give
def _edge_problems():
    """Tiny hand-built LPs: ``[(name, 8-tuple)]``."""
    inf = np.inf
    a_in = scipy.sparse.csr_matrix(np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0]]))
    bu = np.array([1.0, inf])   # the second row has no finite side: b = +inf, y = 0
    c = np.array([1.0, -1.0, 1.0])
    nan_c = np.array([np.nan, -1.0, 1.0])
    one = scipy.sparse.csr_matrix(np.array([[2.0]]))
    return [
        # x0 is free below and meets the row without a finite side only: d_0 = c_0 = 1 > 0 for ever, the bound is -inf
        ("free_variable", (c, None, None, a_in, None, bu, np.array([-inf, 0.0, 0.0]), np.ones(3))),
        ("row_without_a_side", (c, None, None, a_in, None, bu, np.array([-1.0, 0.0, 0.0]), np.ones(3))),
        ("nan_cost", (nan_c, None, None, a_in, None, bu, np.array([-1.0, 0.0, 0.0]), np.ones(3))),
        ("equalities_only", (np.array([1.0, 2.0]), scipy.sparse.csr_matrix(np.array([[1.0, 1.0]])), np.array([1.0]), None, None, None,
                             np.zeros(2), np.ones(2))),
        ("one_variable_one_row", (np.array([-1.0]), None, None, one, None, np.array([1.0]), np.zeros(1), np.ones(1))),
        ("two_sided", (np.array([1.0, -2.0]), scipy.sparse.csr_matrix(np.array([[1.0, -1.0]])), np.array([0.25]),
                       scipy.sparse.csr_matrix(np.array([[1.0, 1.0]])), np.array([0.5]), np.array([1.5]), np.zeros(2), np.ones(2))),
    ]


EDGE_ITERATIONS = 150
EDGE_TOL = (1e-3, 1e-3)


@functools.lru_cache(maxsize=None)
def _edge_reference():
    """Per edge LP the oracle's iterates and the restatement's certificates (shared, read only)."""
    out = []
    for _, p in _edge_problems():
        with np.errstate(invalid="ignore", over="ignore"):
            xs, ys = cp_gap_cpu.iterates(p, EDGE_ITERATIONS)
        out.append((xs, ys, cp_gap_cpu.certificates(p, xs, ys)))
    return out


@pytest.mark.parametrize("form", [None, "global"])
def test_the_decision_is_the_one_the_devices_own_numbers_give(form_env, form):  # noqa: F811
    """Every LP, every evaluated check: one ``iterate(1)`` at a time at ``check_every = 1``, on the fixtures, the edge LPs and the
    seeded random list together."""
    form_env(form)
    problems = [_fixture_problem(c) for c in CASES] + [p for _, p in _edge_problems()] + list(random_problems())
    st = _make(problems)
    try:
        st.set_stop_gap(TOL_GAP, TOL_FEAS, 1)
        running = np.ones(st.count, dtype=bool)
        stops = 0
        for t in range(1, 121):
            st.iterate(1)
            iterations, stopped, primal, bound, violation = st.gap_state()
            assert np.array_equal(iterations[running], np.full(running.sum(), t))
            for k in np.nonzero(running)[0]:
                assert _host_decision(primal[k], bound[k], violation[k], TOL_GAP, TOL_FEAS) == stopped[k], (k, t)
            assert stopped[~running].all()
            stops += int((stopped & running).sum())
            running &= ~stopped
        assert stops >= 10 and running.sum() >= 5
    finally:
        st.close()


# ------------------------------------------------------------------ 3. the split path
@pytest.mark.parametrize("form", [None, "global"])
@pytest.mark.parametrize("every", [1, 4])
def test_split_iterations_give_the_state_and_the_records_of_whole_ones(form_env, every, form):  # noqa: F811
    form_env(form)
    problems = [_fixture_problem(c) for c in CASES] + [p for _, p in _edge_problems()]
    whole, split = _make(problems), _make(problems)
    try:
        for st in (whole, split):
            st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        for t in range(1, 81):
            whole.iterate(1)
            split.primal_step()
            split.dual_step()
            if t % 4 == 0 or t > 40:
                for a, b in zip(whole.gap_state(), split.gap_state()):
                    assert np.array_equal(a, b, equal_nan=True), t
        assert whole.gap_state()[1].sum() >= 2
        for a, b in zip(whole.x() + whole.y(), split.x() + split.y()):
            assert np.array_equal(a, b, equal_nan=True)
        np.testing.assert_array_equal(whole.report()[:, 2:], split.report()[:, 2:])
    finally:
        whole.close()
        split.close()


# ------------------------------------------------------------------ 4. the same records in every form and launch length
def _records_of(form_env, form, kmax, problems, every, total):  # noqa: F811
    form_env(form, kmax)
    st = _make(problems)
    try:
        st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        _advance(st, total, PIECES)
        return st.gap_state(), st.x(), st.y()
    finally:
        st.close()


def test_the_records_do_not_depend_on_the_form_or_the_launch_length(form_env):  # noqa: F811
    problems = [_fixture_problem(c) for c in CASES] + [p for _, p in _edge_problems()] + list(random_problems())
    runs = [_records_of(form_env, form, kmax, problems, RANDOM_EVERY, RANDOM_ITERATIONS)
            for form, kmax in (("lds", None), ("global", None), ("lds", 1), ("global", 7))]
    for state, xs, ys in runs[1:]:
        for a, b in zip(runs[0][0], state):
            assert np.array_equal(a, b, equal_nan=True)
        for a, b in zip(runs[0][1] + runs[0][2], xs + ys):
            assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------ 5. edge LPs
@pytest.mark.parametrize("form", [None, "global"])
def test_edge_lps(form_env, form):  # noqa: F811
    form_env(form)
    names = [name for name, _ in _edge_problems()]
    ref = _edge_reference()
    certs = [cert for _, _, cert in ref]
    for name, cert in zip(names, certs):
        assert cp_gap_cpu.all_decidable(cert, *EDGE_TOL, 1, EDGE_ITERATIONS), name
    want = _expected(certs, 1, EDGE_ITERATIONS, EDGE_TOL)
    by_name = {name: tuple(col[k] for col in want) for k, name in enumerate(names)}
    # what the list is there for, on the restatement
    assert not by_name["free_variable"][1] and by_name["free_variable"][3] == -np.inf
    assert by_name["row_without_a_side"][1] and np.isfinite(by_name["row_without_a_side"][3])
    assert not by_name["nan_cost"][1] and np.isnan(by_name["nan_cost"][2])
    assert by_name["equalities_only"][1] and by_name["one_variable_one_row"][1] and by_name["two_sided"][1]
    st = _make([p for _, p in _edge_problems()])
    try:
        st.set_stop_gap(*EDGE_TOL, 1)
        _advance(st, EDGE_ITERATIONS, PIECES)
        got = st.gap_state()
        _assert_gap_state(got, want)
        assert got[3][names.index("free_variable")] == -np.inf
        xs, ys = st.x(), st.y()
        for k, (rx, ry, _) in enumerate(ref):
            assert np.array_equal(xs[k], rx[want[0][k]], equal_nan=True), names[k]
            assert np.array_equal(ys[k], ry[want[0][k]], equal_nan=True), names[k]
    finally:
        st.close()


def test_an_lp_wider_than_its_workgroup(form_env):  # noqa: F811
    """potts50: 7400 variables on 1024 lanes, the global form by its size; ``tol = 0`` for 40 iterations, every one a check."""
    total = 40
    problem = _fixture_problem("potts50")
    xs, ys = cp_gap_cpu.iterates(problem, total)
    cert = cp_gap_cpu.certificates(problem, xs, ys)
    assert cp_gap_cpu.all_decidable(cert, 0.0, 0.0, 1, total)
    want = _expected([cert], 1, total, (0.0, 0.0))
    assert not want[1][0]
    st = _make([problem])
    try:
        assert st.form(0) == "global" and st.n[0] == 7400
        st.set_stop_gap(0.0, 0.0, 1)
        _advance(st, total, (3, 1, 7))
        _assert_gap_state(st.gap_state(), want)
        assert np.array_equal(st.x()[0], xs[total]) and np.array_equal(st.y()[0], ys[total])
    finally:
        st.close()


# ------------------------------------------------------------------ 6. arming
def test_step_test_then_gap_test_then_off(form_env):  # noqa: F811
    first, more = 50, 170   # the step test at 1e-2 has stopped sc105 (47) and random0 (42) by then
    certs = [fixture_certificates(c, 300) for c in CASES]
    st = _make([_fixture_problem(c) for c in CASES])
    try:
        assert all(np.array_equal(a, b) for a, b in zip(st.gap_state()[2:], (np.full(6, np.inf), np.full(6, -np.inf), np.full(6, np.inf))))
        st.set_stop(1e-2, 1)
        _advance(st, first, PIECES)
        step_state = st.stop_state()
        assert step_state[1].any() and not step_state[1].all()
        st.set_stop_gap(TOL_GAP, TOL_FEAS, 1)   # disarms the step test, clears the flags, keeps the counters
        armed = st.gap_state()
        assert not armed[1].any() and np.array_equal(armed[0], step_state[0]) and np.isinf(armed[2]).all()
        assert np.array_equal(st.stop_state()[2], step_state[2])
        _advance(st, more, PIECES)
        rows = [cp_gap_cpu.gap_state(cert, TOL_GAP, TOL_FEAS, 1, int(t0) + more, after=int(t0)) for cert, t0 in zip(certs, step_state[0])]
        want = tuple(np.array(col) for col in zip(*rows))
        got = st.gap_state()
        _assert_gap_state(got, want)
        assert got[1].sum() >= 3
        again = st.stop_state()
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and np.array_equal(again[2], step_state[2])
        _assert_fixture_iterates(st, CASES, got[0])
        # a stopped LP is not touched: x, y, and through the report z and x4
        st.primal_step()
        rep0 = st.report()
        st.dual_step()
        x0, y0, state0 = st.x(), st.y(), st.gap_state()
        _advance(st, 50, (3, 1, 7))
        st.primal_step()
        rep1 = st.report()
        st.dual_step()
        x1, y1, state1 = st.x(), st.y(), st.gap_state()
        for k in np.nonzero(state0[1])[0]:
            assert np.array_equal(x1[k], x0[k]) and np.array_equal(y1[k], y0[k]) and np.array_equal(rep1[k], rep0[k]), CASES[k]
            assert all(np.array_equal(a[k], b[k]) for a, b in zip(state0, state1))
        assert np.array_equal(state1[0][~state0[1]], state0[0][~state0[1]] + 51)
        # re-arming clears the flags and keeps the counters; off: every LP runs
        st.set_stop_gap(None, None)
        cleared = st.gap_state()
        assert not cleared[1].any() and np.array_equal(cleared[0], state1[0])
        st.iterate(5)
        after = st.gap_state()
        assert np.array_equal(after[0], state1[0] + 5) and not after[1].any()
        assert all(np.array_equal(a, b) for a, b in zip(after[2:], cleared[2:]))   # no check while it is off
        _assert_fixture_iterates(st, CASES, after[0])
    finally:
        st.close()


def test_the_c_abi_refuses_a_bad_tolerance_or_cadence(form_env):  # noqa: F811
    from pysparselp_amd import SlpError, _lib

    st = _make([_fixture_problem("random0")])
    try:
        for tol_gap, tol_feas, every in ((float("nan"), 0.0, 1), (float("inf"), 0.0, 1), (1e-2, -1.0, 1), (1e-2, float("nan"), 1),
                                         (1e-2, 1e-2, 0)):
            with pytest.raises(SlpError, match="slp_many_cpgap_set_stop"):
                _lib.check(st._l.slp_many_cpgap_set_stop(st._h, tol_gap, tol_feas, every))
        _lib.check(st._l.slp_many_cpgap_set_stop(st._h, -1.0, -1.0, 0))   # off: nothing else is looked at
        _lib.check(st._l.slp_many_cpgap_state(st._h, None, None, None, None, None))
    finally:
        st.close()


# ------------------------------------------------------------------ 7. the drivers
def _rowless():
    c = np.array([1.0, -2.0, 0.0])
    return (c, None, None, scipy.sparse.csr_matrix((0, 3)), None, np.zeros(0), -np.ones(3), 2 * np.ones(3))


@pytest.mark.parametrize("cases, every", [(("potts8", "random0", "random2"), 1), (CASES, 10)])
def test_the_list_driver(form_env, cases, every):  # noqa: F811
    from pysparselp_amd import chambolle_pock_ppd_many_certified

    problems = [_fixture_problem(c) for c in cases]
    problems.insert(1, _rowless())
    solved = [0] + list(range(2, len(problems)))
    want = _expected([fixture_certificates(c) for c in cases], every, ITERATIONS)
    rec = InfoRecorder()
    xs, best, info = chambolle_pock_ppd_many_certified(problems, TOL_GAP, TOL_FEAS, every, nb_max_iter=ITERATIONS, callback_func=rec,
                                                       nb_iter_plot=10)
    assert sorted(info) == sorted(NAMES) and rec.info is info and len(best) == len(problems)
    _assert_gap_state(tuple(info[name][solved] for name in NAMES), want)
    assert info["iterations"][1] == 0 and info["stopped"][1] and info["primal"][1] == info["lower_bound"][1] == -1.0 - 4.0
    assert info["violation"][1] == 0.0 and np.array_equal(xs[1], [-1.0, 2.0, 0.0])
    if want[1].all():   # the first report index at which every LP is stopped gets no callback
        last = int(want[0].max())
        assert last < ITERATIONS - 10 and rec.it == list(range(0, last, 10))
    else:
        assert rec.it == list(range(0, ITERATIONS, 10))
    for k, c in zip(solved, cases):
        i = cases.index(c)
        rx, _ = _fixture_iterates(c)
        assert np.array_equal(xs[k], rx[want[0][i]]), c
        for j, niter in enumerate(rec.it):
            is_stopped = bool(want[1][i]) and want[0][i] <= niter
            assert rec.seen[j]["stopped"][k] == is_stopped, (c, niter)
            assert rec.seen[j]["iterations"][k] == (want[0][i] if is_stopped else niter)
            if is_stopped:   # its final iterate, and the last row it had while it was running
                assert np.array_equal(rec.x[j][k], xs[k])
                assert all(store[j][k] == store[j - 1][k] for store in (rec.e1, rec.e2, rec.veq, rec.vineq))
    assert all(seen["stopped"][1] and seen["iterations"][1] == 0 for seen in rec.seen)


@pytest.mark.parametrize("every", [10, 1])
def test_solve_many_certified_equals_solve_for_each_lps_own_count(form_env, every):  # noqa: F811
    from pysparselp_amd import ORDER_SEQUENTIAL, solve_many_certified

    lps, singles = _golden_lps(), _golden_lps()
    xs, elapsed = solve_many_certified(lps, TOL_GAP, TOL_FEAS, check_every=every, nb_iter=ITERATIONS, nb_iter_plot=10)
    assert elapsed > 0 and len(xs) == len(lps)
    print("iterations", [lp.nb_iterations for lp in lps], "stopped", [lp.stopped for lp in lps])
    assert not lps[0].stopped and lps[0].nb_iterations == ITERATIONS and not lps[3].stopped   # sc50a, sc105
    assert lps[1].stopped and lps[4].stopped
    for k, lp in enumerate(singles):
        got = lps[k]
        # the restatement on the LP the solver holds: after remove_fixed_variables
        reduced = copy.deepcopy(lp)
        free, _ = reduced.remove_fixed_variables()
        problem = (reduced.costsvector, reduced.a_equalities, reduced.b_equalities, reduced.a_inequalities, reduced.b_lower,
                   reduced.b_upper, reduced.lower_bounds, reduced.upper_bounds)
        cert = cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, ITERATIONS))
        assert cp_gap_cpu.all_decidable(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS), k
        want = cp_gap_cpu.gap_state(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS)
        assert (got.nb_iterations, got.stopped, got.max_violation) == (want[0], want[1], want[4]), k
        np.testing.assert_allclose([got.primal_objective, got.lower_bound], want[2:4], **ENERGY_TOL)
        fixed_cost = float(np.dot(lp.costsvector[~free], lp.lower_bounds[~free]))
        assert got.fixed_cost == fixed_cost and (fixed_cost != 0.0) == (k == 2)
        x, _ = lp.solve(method="chambolle_pock_ppd", nb_iter=got.nb_iterations, nb_iter_plot=10, order=ORDER_SEQUENTIAL, setup="host")
        assert x.shape == (lp.nb_variables,) and np.array_equal(xs[k], x), k
        # the last check is the last iteration here: primal is the cost of the returned iterate over the free variables
        np.testing.assert_allclose(got.primal_objective, np.dot(lp.costsvector[free], xs[k][free]), **ENERGY_TOL)
        assert got.itrn_curve == lp.itrn_curve == list(range(0, got.nb_iterations, 10))


def test_solve_many_certified_takes_an_lp_without_rows(form_env):  # noqa: F811
    from conftest import load_golden, lp_from_golden
    from pysparselp_amd import solve_many_certified
    from pysparselp_amd.SparseLP import SparseLP

    n = 4
    bare = SparseLP()
    bare.nb_variables = n
    bare.costsvector = np.array([1.0, -2.0, 0.5, 3.0])
    bare.lower_bounds = np.array([-1.0, -1.0, 0.25, -1.0])
    bare.upper_bounds = np.array([2.0, 2.0, 0.25, 2.0])   # variable 2 is fixed
    bare.is_integer = np.zeros(n, dtype=bool)
    bare.a_equalities, bare.b_equalities = scipy.sparse.csr_matrix((0, n)), np.zeros(0)
    bare.a_inequalities, bare.b_lower, bare.b_upper = scipy.sparse.csr_matrix((0, n)), None, np.zeros(0)
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP), bare]
    xs = solve_many_certified(lps, TOL_GAP, TOL_FEAS, check_every=1, get_timing=False, nb_iter=ITERATIONS)
    assert lps[0].stopped and lps[0].nb_iterations == 60
    assert bare.stopped and bare.nb_iterations == 0 and bare.max_violation == 0.0
    assert bare.primal_objective == bare.lower_bound == 1.0 * -1.0 + -2.0 * 2.0 + 3.0 * -1.0   # the vertex of the three free variables
    assert bare.fixed_cost == 0.5 * 0.25
    assert np.array_equal(xs[1][[0, 1, 3]], [-1.0, 2.0, -1.0])


# ------------------------------------------------------------------ 8. a seeded random list
@pytest.mark.parametrize("form, kmax", [(None, None), ("global", 7)])
def test_a_seeded_random_list(form_env, form, kmax):  # noqa: F811
    form_env(form, kmax)
    problems, certs, left_out = random_problems(), random_certificates(), random_left_out()
    keep = np.array([k not in left_out for k in range(len(problems))])
    assert (~keep).sum() <= 2
    want = _expected(certs, RANDOM_EVERY, RANDOM_ITERATIONS)
    st = _make(list(problems))
    try:
        st.set_stop_gap(TOL_GAP, TOL_FEAS, RANDOM_EVERY)
        _advance(st, RANDOM_ITERATIONS, PIECES)
        got = st.gap_state()
        _assert_gap_state(got, want, keep)
        assert len(set(want[0][want[1] & keep])) >= 4 and (~want[1]).any()
        xs, ys = st.x(), st.y()
        for k, p in enumerate(problems):
            if keep[k]:
                rx, ry = cp_gap_cpu.iterates(p, int(want[0][k]))
                assert np.array_equal(xs[k], rx[-1]) and np.array_equal(ys[k], ry[-1]), k
    finally:
        st.close()
