"""The certificate as the per-instance stopping test of the batched Chambolle-Pock solver (csrc/slp_cp_batch.hip:
``CPBatchState.set_stop_gap`` / ``gap_state``, ``chambolle_pock_ppd_batch_certified``, ``SparseLP.solve_batch_certified``) on the GPU.

The violation is a maximum over single-accumulator chains in storage order: compared exactly with the numpy restatement
(tests/cp_gap_cpu.py).  ``primal`` and ``lower_bound`` are sums in the device's fixed order against numpy's: ``rtol = atol = 1e-9``,
``ENERGY_TOL``, the suite's bar for sums in another fixed order.  The stopping iteration and the flag are compared exactly: every
check of every instance used here is decidable, more than 1000 bands of rounding from its threshold, which
tests/test_cp_batch_gap_host.py asserts on the restatement alone.  Every instance's ``x`` and ``y`` are bit for bit those of an
UNARMED batch after exactly that instance's number of iterations.

The references are computed once and shared, never modified.  Needs a real MI355X: run with ``-m gpu``.
"""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse

import cp_gap_cpu
from conftest import load_golden, lp_from_golden
from test_cp_batch_gap_host import (BATCHES, EVERY, ITERATIONS, LARGE, SMALL, TOL_FEAS, TOL_GAP, batch_args, batch_certificates)
from test_gpu_cp_batch import ENERGY_TOL, BatchRecorder, _instances, _of_instance, _run_batch

pytestmark = pytest.mark.gpu

NAMES = ("iterations", "stopped", "primal", "lower_bound", "violation")
PIECES = (7, 1, 32, 3, 50, 64)   # uneven iterate calls; the rest in one more


def _make(args):
    """An unarmed ``CPBatchState`` of the batch ``args``."""
    from pysparselp_amd import CPBatchState
    from pysparselp_amd.ChambollePockPPD import one_sided_system_batch

    a_ineq = args["a_ineq"]
    ineq, b_ineq = (None, None) if a_ineq is None else one_sided_system_batch(a_ineq, args["b_lower"], args["b_upper"])
    return CPBatchState(args["c"], args["a_eq"], args["beq"], ineq, b_ineq, args["lb"], args["ub"], args["x0"], 1, 1)


def _advance(state, k, pieces=PIECES):
    for p in pieces:
        p = min(p, k)
        state.iterate(p)
        k -= p
    state.iterate(k)


def _expected(certs, every, total, tol=(TOL_GAP, TOL_FEAS), after=0):
    """The columns of ``gap_state`` from the restatement."""
    rows = [cp_gap_cpu.gap_state(cert, tol[0], tol[1], every, total, after=after) for cert in certs]
    return tuple(np.array(col) for col in zip(*rows))


def _assert_gap_state(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == bool and all(v.dtype == np.float64 for v in got[2:])
    for name, g, w in zip(NAMES, got, want):
        print(name, g, "expected", w)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[4], want[4], equal_nan=True)
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(got[2], want[2], **ENERGY_TOL)
        np.testing.assert_allclose(got[3], want[3], **ENERGY_TOL)


def _assert_iterates_of_an_unarmed_batch(args, iterations, x, y):
    """Row ``k`` of ``x``, ``y`` is bit for bit that of an unarmed state of the same batch after ``iterations[k]`` iterations: one
    state, stepped through the sorted distinct counts."""
    plain = _make(args)
    try:
        done = 0
        for t in sorted(set(int(v) for v in iterations)):
            _advance(plain, t - done, (5, 1, 40))
            done = t
            rows = np.nonzero(iterations == t)[0]
            px, py = plain.x(), plain.y()
            assert np.array_equal(x[rows], px[rows], equal_nan=True), (t, rows)
            assert np.array_equal(y[rows], py[rows], equal_nan=True), (t, rows)
        first = plain.gap_state()   # a state that was never armed: the count, and no certificate
        assert np.array_equal(first[0], np.full(len(iterations), done)) and not first[1].any()
        assert np.isposinf(first[2]).all() and np.isneginf(first[3]).all() and np.isposinf(first[4]).all()
    finally:
        plain.close()


# ------------------------------------------------------------------ 1. stopping iterations, records and iterates
@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("name", SMALL + LARGE)
def test_every_instance_stops_where_the_restatement_says(name, every):
    args = batch_args(name)
    want = _expected(batch_certificates(name), every, ITERATIONS)
    st = _make(args)
    try:
        assert st.batch == BATCHES[name][1]
        st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        _advance(st, ITERATIONS)
        got = st.gap_state()
        _assert_gap_state(got, want)
        _assert_iterates_of_an_unarmed_batch(args, want[0], st.x(), st.y())
    finally:
        st.close()


@pytest.mark.parametrize("batch, total", [(3, 24), (65, 12), (193, 8)])
def test_more_rows_than_slices(batch, total):
    """potts50, 7400 variables: a slice of a certificate pass holds several rows and columns.  A batch of 3 has 4096 slices and one
    of 65 has 2048, both in scratch of the test's own; 193 instances (four tiles) use the report's 1024 and its scratch.  Both
    tolerances 0, every iteration a check: no instance stops, and the records are those of the restatement."""
    args = _instances(load_golden("lp_potts50"), batch, 5, ("c", "x0"))
    certs = []
    for k in range(batch):
        problem, x0 = _of_instance(args, k)
        certs.append(cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, total, x0)))
        assert cp_gap_cpu.all_decidable(certs[-1], 0.0, 0.0, 1, total), k
    want = _expected(certs, 1, total, (0.0, 0.0))
    assert not want[1].any()
    st = _make(args)
    try:
        assert st.n == 7400
        st.set_stop_gap(0.0, 0.0, 1)
        _advance(st, total, (3, 1, 7))
        _assert_gap_state(st.gap_state(), want)
        _assert_iterates_of_an_unarmed_batch(args, want[0], st.x(), st.y())
    finally:
        st.close()


# ------------------------------------------------------------------ 2. the decision is the one the device's own numbers give
def _edge_args():
    """One matrix with a variable free below (x0, which meets only the row without a finite side) and four costs: ``d_0 = c_0 = 1 >
    0`` for ever, so the bound is ``-inf``; a NaN cost; ``c_0 < 0``, ordinary; ``c_0 = 0``, whose term is left out."""
    inf = np.inf
    a_in = scipy.sparse.csr_matrix(np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 0.0]]))
    c = np.array([[1.0, -1.0, 1.0], [np.nan, -1.0, 1.0], [-1.0, -1.0, 1.0], [0.0, -1.0, 1.0]])
    return dict(c=c, a_eq=None, beq=None, a_ineq=a_in, b_lower=None, b_upper=np.array([1.0, inf]), lb=np.array([-inf, 0.0, 0.0]),
                ub=np.ones(3), x0=None)


EDGE_NAMES = ("minus_inf_bound", "nan_cost", "ordinary", "zero_cost")
EDGE_ITERATIONS = 150
EDGE_TOL = (1e-3, 1e-3)


@functools.lru_cache(maxsize=None)
def _edge_certificates():
    out = []
    args = _edge_args()
    for k in range(len(EDGE_NAMES)):
        problem, x0 = _of_instance(args, k)
        with np.errstate(invalid="ignore", over="ignore"):
            out.append(cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, EDGE_ITERATIONS, x0)))
    return tuple(out)


@pytest.mark.parametrize("batch", ["potts8_65", "edge"])
def test_the_decision_is_the_one_the_devices_own_numbers_give(batch):
    """Every running instance, every evaluated check: one ``iterate(1)`` at a time at ``check_every = 1``; a stopped instance never
    changes again -- records, ``x`` and ``y``."""
    args, tol = (_edge_args(), EDGE_TOL) if batch == "edge" else (batch_args(batch), (TOL_GAP, TOL_FEAS))
    st = _make(args)
    try:
        st.set_stop_gap(*tol, 1)
        running = np.ones(st.batch, dtype=bool)
        frozen = {}
        for t in range(1, 121):
            st.iterate(1)
            state = st.gap_state()
            iterations, stopped, primal, bound, violation = state
            assert np.array_equal(iterations[running], np.full(running.sum(), t))
            for k in np.nonzero(running)[0]:
                assert cp_gap_cpu.decision(primal[k], bound[k], violation[k], *tol) == stopped[k], (k, t)
            assert stopped[~running].all()
            new = np.nonzero(stopped & running)[0]
            if new.size or t % 40 == 0:
                x, y = st.x(), st.y()
                for k, (rec, fx, fy) in frozen.items():
                    assert all(np.array_equal(a[k], b, equal_nan=True) for a, b in zip(state, rec)), (k, t)
                    assert np.array_equal(x[k], fx) and np.array_equal(y[k], fy), (k, t)
                for k in new:
                    frozen[int(k)] = (tuple(col[k] for col in state), x[k].copy(), y[k].copy())
            running &= ~stopped
        if batch == "edge":
            assert list(running) == [True, True, False, False]
        else:
            assert not running.any() and len(set(st.gap_state()[0])) >= 20
    finally:
        st.close()


# ------------------------------------------------------------------ 3. edge instances
def test_edge_instances():
    certs = _edge_certificates()
    for name, cert in zip(EDGE_NAMES, certs):
        assert cp_gap_cpu.all_decidable(cert, *EDGE_TOL, 1, EDGE_ITERATIONS), name
    want = _expected(certs, 1, EDGE_ITERATIONS, EDGE_TOL)
    by_name = {name: tuple(col[k] for col in want) for k, name in enumerate(EDGE_NAMES)}
    # what the batch is there for, on the restatement
    assert not by_name["minus_inf_bound"][1] and by_name["minus_inf_bound"][3] == -np.inf
    assert not by_name["nan_cost"][1] and np.isnan(by_name["nan_cost"][2])
    assert by_name["ordinary"][1] and by_name["zero_cost"][1]
    args = _edge_args()
    st = _make(args)
    try:
        st.set_stop_gap(*EDGE_TOL, 1)
        _advance(st, EDGE_ITERATIONS)
        got = st.gap_state()
        _assert_gap_state(got, want)
        assert got[3][0] == -np.inf and np.isnan(got[2][1])
        for k in (2, 3):   # no record of a neighbour holds a NaN
            assert all(np.isfinite(col[k]) for col in got[2:]), k
        _assert_iterates_of_an_unarmed_batch(args, want[0], st.x(), st.y())
    finally:
        st.close()


# ------------------------------------------------------------------ 4. the split path
@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("name", ["potts8_c", "potts8_65"])
def test_split_iterations_give_the_state_and_the_records_of_whole_ones(name, every):
    args = batch_args(name)
    whole, split = _make(args), _make(args)
    try:
        for st in (whole, split):
            st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        for t in range(1, 81):
            whole.iterate(1)
            split.primal_step()
            split.dual_step()
            if t % 4 == 0 or t > 48:
                for a, b in zip(whole.gap_state(), split.gap_state()):
                    assert np.array_equal(a, b), t
        assert whole.gap_state()[1].sum() >= 2
        assert np.array_equal(whole.x(), split.x()) and np.array_equal(whole.y(), split.y())
    finally:
        whole.close()
        split.close()


# ------------------------------------------------------------------ 5. armed late, re-armed, disarmed
def test_armed_late_then_rearmed_then_disarmed():
    name, after, first, more = "potts8_c", 7, 62, 20
    args, certs = batch_args(name), batch_certificates(name)
    st, plain = _make(args), _make(args)
    try:
        st.iterate(after)   # unarmed: counted
        st.set_stop_gap(TOL_GAP, TOL_FEAS, 4)
        armed = st.gap_state()
        assert np.array_equal(armed[0], np.full(5, after)) and not armed[1].any() and np.isposinf(armed[2]).all()
        _advance(st, first - after, (3, 1, 7))
        want = _expected(certs, 4, first, after=after)   # checks at t % 4 == 0 of the life count
        got = st.gap_state()
        _assert_gap_state(got, want)
        assert list(want[1]) == [True, False, False, False, False] and want[0][0] == 60
        # tolerance 0 from here on: the stopped instance stays stopped, the rest never stop
        st.set_stop_gap(0.0, 0.0, 1)
        kept = st.gap_state()
        assert all(np.array_equal(a, b) for a, b in zip(kept, got))
        _advance(st, more, (3, 1, 7))
        got = st.gap_state()
        rows = [cp_gap_cpu.gap_state(cert, 0.0, 0.0, 1, first + more, after=first) for cert in certs[1:]]
        assert all(not row[1] for row in rows)
        assert all(cp_gap_cpu.all_decidable(cert, 0.0, 0.0, 1, first + more, after=first) for cert in certs[1:])
        _assert_gap_state(tuple(col[1:] for col in got), tuple(np.array(col) for col in zip(*rows)))
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(got, kept))
        # disarmed: the stopped one stays frozen, the others are the unarmed batch and no certificate is evaluated
        st.set_stop_gap(None, None)
        _advance(st, 25, (3, 1, 7))
        off = st.gap_state()
        assert off[1][0] and off[0][0] == 60 and np.array_equal(off[0][1:], np.full(4, first + more + 25)) and not off[1][1:].any()
        assert all(np.array_equal(a, b) for a, b in zip(off[2:], got[2:]))
        _assert_iterates_of_an_unarmed_batch(args, off[0], st.x(), st.y())
        plain.set_stop_gap(None, None)   # on a state that was never armed: nothing
        plain.iterate(3)
        assert np.array_equal(plain.gap_state()[0], np.full(5, 3)) and not plain.gap_state()[1].any()
    finally:
        st.close()
        plain.close()


def test_the_c_abi_refuses_a_bad_tolerance_or_cadence():
    from pysparselp_amd import SlpError, _lib

    st = _make(batch_args("potts8_1"))
    try:
        for tol_gap, tol_feas, every in ((float("nan"), 0.0, 1), (float("inf"), 0.0, 1), (1e-2, -1.0, 1), (1e-2, float("nan"), 1),
                                         (1e-2, 1e-2, 0)):
            with pytest.raises(SlpError, match="slp_cp_batch_set_stop_gap"):
                _lib.check(st._l.slp_cp_batch_set_stop_gap(st._h, tol_gap, tol_feas, every))
        _lib.check(st._l.slp_cp_batch_set_stop_gap(st._h, -1.0, -1.0, 0))   # off: nothing else is looked at
        _lib.check(st._l.slp_cp_batch_gap_state(st._h, None, None, None, None, None))
    finally:
        st.close()


# ------------------------------------------------------------------ 6. all stopped: nothing is launched
def test_a_wholly_stopped_batch_launches_nothing():
    name = "potts8_65"
    st = _make(batch_args(name))
    try:
        st.set_stop_gap(TOL_GAP, TOL_FEAS, 1)
        _advance(st, 120)
        before = st.gap_state()
        assert before[1].all() and before[0].max() == 100
        st.primal_step()
        rep = st.report()
        st.dual_step()
        x, y = st.x(), st.y()
        st.iterate(50)
        st.primal_step()
        st.dual_step()
        assert all(np.array_equal(a, b) for a, b in zip(st.gap_state(), before))
        assert np.array_equal(st.x(), x) and np.array_equal(st.y(), y)
        st.primal_step()
        assert np.array_equal(st.report(), rep)   # z and x4 too
        st.dual_step()
        st.set_stop_gap(None, None)   # disarmed: still stopped, the count of iterations stays
        st.iterate(5)
        assert all(np.array_equal(a, b) for a, b in zip(st.gap_state(), before))
        _assert_iterates_of_an_unarmed_batch(batch_args(name), before[0], x, y)
    finally:
        st.close()


# ------------------------------------------------------------------ 7. an instance does not depend on its batch
def test_the_first_instances_of_a_large_batch_as_a_batch_of_their_own():
    args = batch_args("potts8_65")
    few = {k: (v[:5] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in args.items()}
    large, small = _make(args), _make(few)
    try:
        for st in (large, small):
            st.set_stop_gap(TOL_GAP, TOL_FEAS, 4)
            _advance(st, ITERATIONS)
        a, b = large.gap_state(), small.gap_state()
        assert small.batch == 5 and b[1].all()
        for i in (0, 1, 4):
            assert np.array_equal(a[i][:5], b[i]), NAMES[i]
        np.testing.assert_allclose(a[2][:5], b[2], **ENERGY_TOL)   # another number of slices
        np.testing.assert_allclose(a[3][:5], b[3], **ENERGY_TOL)
        assert np.array_equal(large.x()[:5], small.x()) and np.array_equal(large.y()[:5], small.y())
    finally:
        large.close()
        small.close()


# ------------------------------------------------------------------ 8. against the list solver
@pytest.mark.parametrize("every", [1, 10])
def test_the_batch_and_the_list_solver_stop_alike(every):
    """The same five potts8 LPs through the two kernel families on one device."""
    from test_gpu_cp_many_stop import _make as make_list

    args = batch_args("potts8_c")
    st, ls = _make(args), make_list([_of_instance(args, k)[0] for k in range(5)])
    try:
        st.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        ls.set_stop_gap(TOL_GAP, TOL_FEAS, every)
        _advance(st, ITERATIONS)
        _advance(ls, ITERATIONS)
        a, b = st.gap_state(), ls.gap_state()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].all() and np.array_equal(a[4], b[4])
        np.testing.assert_allclose(a[2], b[2], **ENERGY_TOL)
        np.testing.assert_allclose(a[3], b[3], **ENERGY_TOL)
        for k, (lx, ly) in enumerate(zip(ls.x(), ls.y())):
            assert np.array_equal(st.x()[k], lx) and np.array_equal(st.y()[k], ly), k
    finally:
        st.close()
        ls.close()


# ------------------------------------------------------------------ 9. the drivers
class InfoRecorder(BatchRecorder):
    """Also keeps the ``info`` the driver sets as an attribute of its callback, as it is at every call."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __call__(self, *report):
        super().__call__(*report)
        self.seen.append({name: values.copy() for name, values in self.info.items()})


def _certified(args, *stop, **kw):
    from pysparselp_amd import chambolle_pock_ppd_batch_certified

    return chambolle_pock_ppd_batch_certified(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"],
                                              args["lb"], args["ub"], *stop, x0=args["x0"], **kw)


@pytest.mark.parametrize("every", [1, 10])
def test_the_batch_driver(every):
    name = "potts8_c"
    args = batch_args(name)
    want = _expected(batch_certificates(name), every, ITERATIONS)
    rec = InfoRecorder()
    x, best, info = _certified(args, TOL_GAP, TOL_FEAS, every, nb_max_iter=ITERATIONS, callback_func=rec, nb_iter_plot=10)
    assert sorted(info) == sorted(NAMES) and rec.info is info and len(best) == 5 and x.shape == args["c"].shape
    _assert_gap_state(tuple(info[n] for n in NAMES), want)
    last = int(want[0].max())   # the first report index at which every instance is stopped gets no callback
    assert want[1].all() and last < ITERATIONS - 10 and rec.it == list(range(0, last, 10))
    for j, niter in enumerate(rec.it):
        for k in range(5):
            is_stopped = want[0][k] <= niter
            assert rec.seen[j]["stopped"][k] == is_stopped and rec.seen[j]["iterations"][k] == (want[0][k] if is_stopped else niter)
            if is_stopped:   # its final iterate, and the last row it had while it was running
                assert np.array_equal(rec.x[j][k], x[k])
                assert all(store[j][k] == store[j - 1][k] for store in (rec.e1, rec.e2, rec.veq, rec.vineq))
    for t in sorted(set(int(v) for v in want[0])):
        plain, _ = _run_batch(args, nb_max_iter=t, nb_iter_plot=10)
        rows = np.nonzero(want[0] == t)[0]
        assert np.array_equal(x[rows], plain[rows]), t
    # max_time = 0 stops at the first report
    rec = InfoRecorder()
    _, _, info = _certified(args, TOL_GAP, TOL_FEAS, every, nb_max_iter=ITERATIONS, callback_func=rec, max_time=0.0)
    assert rec.it == [] and not info["stopped"].any() and np.array_equal(info["iterations"], np.zeros(5))


@functools.lru_cache(maxsize=None)
def _lp_and_costs():
    """potts8 with one variable fixed through equal bounds, and five rows of costs (row 0 the LP's own)."""
    from pysparselp_amd.SparseLP import SparseLP

    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    lp.lower_bounds[3] = lp.upper_bounds[3] = 1.0
    rs = np.random.RandomState(31)
    costs = np.tile(lp.costsvector, (5, 1))
    costs[1:] = lp.costsvector * (1 + 0.2 * rs.randn(4, lp.nb_variables)) + 0.05 * np.mean(np.abs(lp.costsvector)) * rs.randn(4, lp.nb_variables)
    return lp, costs


@pytest.mark.parametrize("every", [10, 1])
def test_solve_batch_certified_equals_solve_batch_for_each_instances_own_count(every):
    base, costs = _lp_and_costs()
    lp, plain = copy.deepcopy(base), copy.deepcopy(base)
    reduced = copy.deepcopy(base)
    free, _ = reduced.remove_fixed_variables()
    assert (~free).sum() == 1
    x, elapsed = lp.solve_batch_certified(costs, TOL_GAP, TOL_FEAS, check_every=every, nb_iter=ITERATIONS, nb_iter_plot=10)
    info = lp.batch_info
    assert elapsed > 0 and x.shape == costs.shape and sorted(info) == sorted(NAMES + ("fixed_cost",))
    print({name: info[name] for name in info})
    assert np.array_equal(info["fixed_cost"], costs[:, ~free].dot(base.lower_bounds[~free])) and (info["fixed_cost"] != 0).all()
    for k in range(5):   # the restatement on the LP the solver holds: after remove_fixed_variables
        problem = (costs[k][free], reduced.a_equalities, reduced.b_equalities, reduced.a_inequalities, reduced.b_lower, reduced.b_upper,
                   reduced.lower_bounds, reduced.upper_bounds)
        cert = cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, ITERATIONS))
        assert cp_gap_cpu.all_decidable(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS), k
        want = cp_gap_cpu.gap_state(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS)
        assert (info["iterations"][k], info["stopped"][k], info["violation"][k]) == (want[0], want[1], want[4]), k
        np.testing.assert_allclose([info["primal"][k], info["lower_bound"][k]], want[2:4], **ENERGY_TOL)
    assert info["stopped"].any()
    for t in sorted(set(int(v) for v in info["iterations"])):
        px = plain.solve_batch(costs, nb_iter=t, nb_iter_plot=10, get_timing=False)
        rows = np.nonzero(info["iterations"] == t)[0]
        assert np.array_equal(x[rows], px[rows]), t
    # the curves: one row per report, a stopped instance repeats its last running row
    last = int(info["iterations"].max()) if info["stopped"].all() else ITERATIONS
    assert lp.itrn_curve == list(range(0, last, 10))
    for j, niter in enumerate(lp.itrn_curve):
        for k in np.nonzero(info["stopped"] & (info["iterations"] <= niter))[0]:
            if j > 0 and info["iterations"][k] <= lp.itrn_curve[j - 1]:
                assert all(getattr(lp, c)[j][k] == getattr(lp, c)[j - 1][k]
                           for c in ("pobj_curve", "dobj_curve", "max_violated_equality", "max_violated_inequality", "max_violated_constraint"))
