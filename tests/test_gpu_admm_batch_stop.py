"""Per-instance stopping of the batched ADMM solver (csrc/slp_admm_batch.hip: ``ADMMBatchState.set_stop`` / ``stop_state``,
``lp_admm_batch_until``, ``SparseLP.solve_admm_batch_until``) on the GPU, in BOTH forms of the iteration
(``SLP_ADMM_BATCH_FORM``).

The expectations come from the numpy restatement (tests/admm_batch_stop_cpu.py) on the oracle's iterates; the batches and the
conditions that make them a test are those of tests/test_admm_batch_stop_host.py.  Every comparison is exact
(``np.array_equal``): the stopping iterations, the last evaluated residual and step, ``x`` over all ``N`` columns and ``lambda`` of a
stopped instance against the single-instance solver in SEQUENTIAL order after exactly its stopping iteration, a running
instance against the same batch without a test.  The one exception is the report's energy, a sum in another fixed order:
``ENERGY_TOL`` of tests/test_gpu_admm_batch.py.  An instance whose arithmetic overflows to NaN (section 3b) is compared with the oracle's
iterates, NaN for NaN.  Needs a real MI355X: run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest

import admm_batch_stop_cpu
from conftest import load_golden, lp_from_golden
from test_admm_batch_stop_host import (BATCHES, EVERY, NAN_EVERY, NAN_INSTANCE, NAN_TOL, NAN_TOTAL, batch_args, batch_curves, batch_stops, fuzz_batched,
                                       nan_batch)
from test_gpu_admm_batch import ENERGY_TOL, FORMS, _mods, _of_instance, _state, _take

pytestmark = pytest.mark.gpu

PIECES = (3, 1, 7, 50, 64, 30)


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    monkeypatch.setenv("SLP_ADMM_BATCH_FORM", request.param)
    return request.param


@pytest.fixture
def tile4(monkeypatch):
    monkeypatch.setenv("SLP_ADMM_BATCH_TILE", "4")


def _expected(name, schedule=None, total=None, batch=5, order=None):
    """``stop_state`` of the restatement; ``order``: the instances of the batch permuted."""
    curves = batch_curves(name, batch)
    if order is not None:
        curves = tuple(curves[k] for k in order)
    _, _, tol, run = BATCHES[name]
    return admm_batch_stop_cpu.stop_state(curves, tol + (EVERY,) if schedule is None else schedule, run if total is None else total)


def _same_state(got, want, nan=False):
    """``nan``: the restatement itself holds a NaN, which the device must hold in the same place."""
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == np.float64 and got[3].dtype == np.float64
    for g, w, what in zip(got, want, ("iterations", "stopped", "residual", "step")):
        assert np.array_equal(g, w, equal_nan=nan and g.dtype == np.float64), (what, g, w)


@functools.lru_cache(maxsize=None)
def _single(name, batch, k, iters):
    """``(x over all N, lambda)`` of instance ``k`` alone after ``iters`` iterations of the single-instance solver (shared, read
    only)."""
    _, _, ADMMState, seq = _mods()
    (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = _of_instance(batch_args(name, batch), k)
    st = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0, 2, 3, True, order=seq)
    try:
        st.iterate(iters)
        out = st.x(), st.lam()
    finally:
        st.close()
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _untested(name, iters, batch=5):
    """``(x over all N, lambda)`` of the batch after ``iters`` iterations of a state that was never armed (shared, read only)."""
    st = _state(batch_args(name, batch))
    try:
        st.iterate(iters)
        out = st.x(), st.lam()
    finally:
        st.close()
    for v in out:
        v.setflags(write=False)
    return out


def _armed(args, tol, every=EVERY):
    st = _state(args)
    st.set_stop(tol[0], tol[1], every)
    return st


def _check_iterates(st, name, want, total, batch=5, order=None):
    """A stopped instance holds the single solver's iterate of its stopping iteration, a running one the untested batch's."""
    x, lam = st.x(), st.lam()
    for j in range(x.shape[0]):
        k = j if order is None else int(order[j])
        if want[1][j]:
            xs, ls = _single(name, batch, k, int(want[0][j]))
        else:
            xu, lu = _untested(name, total, batch)
            xs, ls = xu[k], lu[k]
        assert np.array_equal(x[j], xs) and np.array_equal(lam[j], ls), (j, k)


# ------------------------------------------------------------------ 1. the fixture batches against the restatement
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_batch_stops_where_the_restatement_does(name, form):
    _, _, tol, total = BATCHES[name]
    stops = batch_stops(name)
    assert len(set(t for t in stops if t is not None)) >= 2
    if name == "potts8_mixed":
        assert any(t is None for t in stops) and any(t is not None for t in stops)
    want = _expected(name)
    st = _armed(batch_args(name), tol)
    try:
        assert st.form() == form
        _same_state(st.stop_state(), _expected(name, total=0))   # +inf before the first test
        st.iterate(total)
        got = st.stop_state()
        print(name, form, got)
        _same_state(got, want)
        _check_iterates(st, name, want, total)
    finally:
        st.close()


# ------------------------------------------------------------------ 2. the split of a run
@pytest.mark.parametrize("name", ["potts8_mixed", "sc105"])
def test_the_result_does_not_depend_on_the_split_of_the_run(name, form):
    _, _, tol, total = BATCHES[name]
    whole, pieces = _armed(batch_args(name), tol), _armed(batch_args(name), tol)
    try:
        whole.iterate(total)
        for k in PIECES + (total - sum(PIECES),):
            assert k > 0
            pieces.iterate(k)
        _same_state(whole.stop_state(), _expected(name))
        _same_state(pieces.stop_state(), _expected(name))
        assert np.array_equal(whole.x(), pieces.x()) and np.array_equal(whole.lam(), pieces.lam())
    finally:
        whole.close()
        pieces.close()


def test_an_iteration_in_two_halves_stops_the_same_instances(form):
    name, total = "sc105", 60
    _, _, tol, _ = BATCHES[name]
    _, _, ADMMState, seq = _mods()
    args = batch_args(name)
    st = _armed(args, tol)
    try:
        for t in range(1, total + 1):
            st.sweep_step()
            if t == EVERY:   # between the halves of the first check iteration: every instance still runs
                rep = st.report()
                for k in range(5):
                    (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = _of_instance(args, k)
                    one = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0, 2, 3, True, order=seq)
                    try:
                        one.iterate(t - 1)
                        one.sweep_step()
                        r = one.report()[:3]
                    finally:
                        one.close()
                    assert np.array_equal(rep[k, 1:], r[1:]), k
                    np.testing.assert_allclose(rep[k, 0], r[0], **ENERGY_TOL)
            st.multiplier_step()
        want = _expected(name, total=total)
        assert want[1].all() and len(set(want[0])) >= 2
        _same_state(st.stop_state(), want)
        _check_iterates(st, name, want, total)
    finally:
        st.close()


# ------------------------------------------------------------------ 3. tile edges (tiles of four instances)
@pytest.mark.parametrize("batch", [5, 1])
def test_tile_edges(batch, form, tile4):
    """B = 5: a full tile -- in which instance 1 stops at 10 while its tile-mates run to 50 -- and a tile of one instance and
    three padding lanes; B = 1: one instance and three padding lanes."""
    name = "sc105"
    _, _, tol, total = BATCHES[name]
    want = _expected(name, batch=batch)
    if batch == 5:
        assert want[0][1] + 2 * EVERY <= max(want[0][0], want[0][2], want[0][3])
    st = _armed(batch_args(name, batch), tol)
    try:
        st.iterate(total)
        _same_state(st.stop_state(), want)
        _check_iterates(st, name, want, total, batch=batch)
    finally:
        st.close()


def test_a_tile_that_stops_long_before_another(form, tile4):
    """Eight instances ordered by their stopping iteration: tile 0 is wholly stopped at least two checks before tile 1 -- its
    workgroup returns at the start of a launch, and inside one."""
    name, batch = "sc105", 8
    _, _, tol, total = BATCHES[name]
    stops = admm_batch_stop_cpu.stopping_iterations(batch_curves(name, batch), *tol, EVERY, total)
    order = np.argsort(stops, kind="stable")
    assert stops[order[3]] + 2 * EVERY <= stops[order[-1]]
    want = _expected(name, batch=batch, order=order)
    for split in ((total,), (stops[order[3]] + 5, total - stops[order[3]] - 5)):   # inside a launch; at the start of one
        st = _armed(_take(batch_args(name, batch), order), tol)
        try:
            for k in split:
                st.iterate(k)
            _same_state(st.stop_state(), want)
            _check_iterates(st, name, want, total, batch=batch, order=order)
        finally:
            st.close()


# ------------------------------------------------------------------ 3b. a NaN never stops
@functools.lru_cache(maxsize=None)
def _nan_references():
    """Per instance of the NaN batch the oracle's iterates over ``NAN_TOTAL`` iterations (``fuzz_batched.StopRef``; shared, read
    only)."""
    args, _ = nan_batch()
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(fuzz_batched.admm_stop_reference(*_of_instance(args, k), NAN_TOTAL, 10 ** 9) for k in range(args["cs"].shape[0]))


@pytest.mark.parametrize("every", NAN_EVERY)
def test_an_instance_that_overflows_never_stops_and_leaves_its_tile_mates_alone(every, form, tile4):
    """Instance 2 of five -- in the middle of a full tile of four, with a tile of one instance behind it -- has a cost of 1e308 on
    a variable without an upper bound: its residual and step are about 1e307, then infinite, then NaN (the conditions are those
    of tests/test_admm_batch_stop_host.py).  The maxima keep a NaN through the shuffles, the LDS slots and the slots of the levels
    form, so the instance never stops under tolerances that a record of 0.0 would meet at once: it runs to the end with the
    NaN in its record from the first check behind it, its iterate the oracle's, NaN for NaN.  The four others stop where the
    restatement says with the oracle's iterates of their own stopping iterations, bit for bit."""
    args, curves = nan_batch()
    bad = np.isnan(curves[NAN_INSTANCE][0]) | np.isnan(curves[NAN_INSTANCE][1])
    first_check = -(-(int(np.argmax(bad)) + 1) // every) * every   # the first check iteration with the NaN
    st = _armed(args, NAN_TOL, every)
    try:
        assert st.form() == form
        st.iterate(first_check)
        got = st.stop_state()
        print(form, every, first_check, got)
        assert np.isnan(got[2][NAN_INSTANCE]) and np.isnan(got[3][NAN_INSTANCE]) and not got[1].any()
        _same_state(got, admm_batch_stop_cpu.stop_state(curves, NAN_TOL + (every,), first_check), nan=True)
        st.iterate(NAN_TOTAL - first_check)
        want = admm_batch_stop_cpu.stop_state(curves, NAN_TOL + (every,), NAN_TOTAL)
        got = st.stop_state()
        print(got)
        assert want[1].sum() == 4 and not got[1][NAN_INSTANCE] and got[0][NAN_INSTANCE] == NAN_TOTAL
        assert np.isnan(got[2][NAN_INSTANCE]) and np.isnan(got[3][NAN_INSTANCE])
        _same_state(got, want, nan=True)
        x, lam = st.x(), st.lam()
        for k, ref in enumerate(_nan_references()):
            t = int(want[0][k])
            assert np.array_equal(x[k], ref.xs[t], equal_nan=k == NAN_INSTANCE), k
            assert np.array_equal(lam[k], ref.duals[t], equal_nan=k == NAN_INSTANCE), k
        assert np.isnan(x[NAN_INSTANCE]).any() and np.all(np.isfinite(np.delete(x, NAN_INSTANCE, axis=0)))
    finally:
        st.close()


# ------------------------------------------------------------------ 4. re-arming, turning off, nothing left to run
def test_rearming_keeps_the_flags_and_turning_off_lets_the_rest_run(form):
    name = "potts8_mixed"
    _, _, tol, total = BATCHES[name]
    tight = (1e-5, 1e-5)
    schedule = [(0,) + tol + (EVERY,), (100,) + tight + (EVERY,)]
    st = _armed(batch_args(name), tol)
    try:
        st.iterate(100)
        first = _expected(name, total=100)
        assert first[1].any() and not first[1].all()
        _same_state(st.stop_state(), first)
        st.set_stop(*tight, EVERY)
        _same_state(st.stop_state(), first)                      # the call itself changes nothing
        st.iterate(50)
        want = _expected(name, schedule, 150)
        assert np.array_equal(want[1], first[1]) and np.array_equal(want[0][first[1]], first[0][first[1]])
        assert not np.array_equal(want[1], _expected(name, total=150)[1])   # under the first tolerances one more had stopped
        _same_state(st.stop_state(), want)
        st.set_stop(None, None)                                  # tol_residual = -1 at the C level
        st.iterate(total - 150)
        want = _expected(name, schedule + [(150, None, None, 1)], total)
        _same_state(st.stop_state(), want)
        _check_iterates(st, name, want, total)
    finally:
        st.close()


def test_nothing_is_enqueued_when_every_instance_is_stopped(form):
    name = "sc105"
    _, _, tol, _ = BATCHES[name]
    want = _expected(name, total=60)
    assert want[1].all()
    st = _armed(batch_args(name), tol)
    try:
        st.iterate(60)
        _same_state(st.stop_state(), want)
        x, lam = st.x(), st.lam()
        st.iterate(7)
        st.sweep_step()
        st.multiplier_step()
        _same_state(st.stop_state(), want)
        assert np.array_equal(st.x(), x) and np.array_equal(st.lam(), lam)
        st.bench(3)                                              # evaluates no test, moves no stopped instance
        _same_state(st.stop_state(), want)
        assert np.array_equal(st.x(), x) and np.array_equal(st.lam(), lam)
    finally:
        st.close()


def test_a_state_that_was_never_armed_is_the_state_of_today(form):
    name, iters = "random1", 40
    st = _state(batch_args(name))
    try:
        st.set_stop(None, None)   # turning off what was never on changes nothing
        st.iterate(iters)
        got = st.stop_state()
        _same_state(got, (np.full(5, iters), np.zeros(5, dtype=bool), np.full(5, np.inf), np.full(5, np.inf)))
        x, lam = st.x(), st.lam()
        for k in range(5):
            xs, ls = _single(name, 5, k, iters)
            assert np.array_equal(x[k], xs) and np.array_equal(lam[k], ls), k
    finally:
        st.close()


# ------------------------------------------------------------------ 5. the solver calls
class _InfoRecorder:
    """The callbacks of ``lp_admm_batch_until``: the index, X, the equality violation and a copy of ``info`` as it is then."""

    def __init__(self):
        self.calls = []

    def __call__(self, niter, sol, e1, e2, dur, veq, vineq):
        self.calls.append((niter, np.array(sol, copy=True), np.array(veq, copy=True), {k: v.copy() for k, v in self.info.items()},
                           self.info))


def _until(name, *stop, **kw):
    from pysparselp_amd import lp_admm_batch_until

    a = batch_args(name)
    return lp_admm_batch_until(a["cs"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"], *stop, x0=a["x0"],
                               **kw)


def test_lp_admm_batch_until(form):
    name = "potts8"
    _, _, tol, total = BATCHES[name]
    stops = batch_stops(name)
    last = max(stops)
    want = _expected(name, total=last)
    assert want[1].all() and last % 10 == 0 and min(stops) < last - 10
    rec = _InfoRecorder()
    X, info = _until(name, *tol, EVERY, nb_iter=total, callback_func=rec, nb_iter_plot=10)
    assert sorted(info) == ["iterations", "residual", "step", "stopped"]
    _same_state(tuple(info[k] for k in ("iterations", "stopped", "residual", "step")), want)
    # the loop ends at the first report index with every instance stopped: no callback for it
    assert [c[0] for c in rec.calls] == list(range(0, last, 10))
    assert all(c[4] is info for c in rec.calls) and rec.info is info
    n = X.shape[1]
    for k in range(5):
        assert np.array_equal(X[k], _single(name, 5, k, stops[k])[0][:n]), k
    # in a callback info is current, and a stopped instance's report is that of its frozen iterate
    early = int(np.argmin(stops))
    seen = 0
    for niter, sol, veq, then, _ in rec.calls:
        _same_state(tuple(then[k] for k in ("iterations", "stopped", "residual", "step")), _expected(name, total=niter))
        if niter >= stops[early]:
            assert then["stopped"][early] and veq[early] == then["residual"][early] == info["residual"][early]
            assert np.array_equal(sol[early], X[early])
            seen += 1
    assert seen >= 1


def test_lp_admm_batch_until_ends_at_the_first_report_when_time_is_up(form):
    name = "potts8"
    rec = _InfoRecorder()
    X, info = _until(name, *BATCHES[name][2], EVERY, nb_iter=50, callback_func=rec, max_time=0)
    assert rec.calls == [] and np.array_equal(info["iterations"], np.zeros(5)) and not info["stopped"].any()
    assert np.all(np.isinf(info["residual"])) and np.all(np.isinf(info["step"]))
    st = _state(batch_args(name))
    try:
        st.sweep_step()
        assert np.array_equal(X, st.x(X.shape[1]))
    finally:
        st.close()


def test_solve_admm_batch_until(form):
    from pysparselp_amd.SparseLP import SparseLP

    name = "potts8"
    _, _, tol, total = BATCHES[name]
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    costs = batch_args(name)["cs"]
    X, elapsed, info = lp.solve_admm_batch_until(costs, *tol, nb_iter=total)
    Xr, want = _until(name, *tol, EVERY, nb_iter=total)
    assert np.array_equal(X, Xr) and elapsed > 0
    for k in want:
        assert np.array_equal(info[k], want[k]), k
    reports = max(batch_stops(name)) // 10
    assert lp.itrn_curve == list(range(0, 10 * reports, 10))
    for curve in (lp.pobj_curve, lp.dobj_curve, lp.max_violated_equality, lp.max_violated_inequality, lp.max_violated_constraint):
        assert len(curve) == reports and all(np.shape(v) == (5,) for v in curve)
    X2, info2 = lp.solve_admm_batch_until(costs, *tol, nb_iter=total, get_timing=False)
    assert np.array_equal(X2, X) and np.array_equal(info2["iterations"], info["iterations"])


# ------------------------------------------------------------------ 6. the refusals of the library
def test_the_library_refuses_a_call_between_the_halves_and_bad_values(form):
    from pysparselp_amd import SlpError, _lib

    name = "sc105"
    st = _state(batch_args(name))
    try:
        call = lambda *a: int(st._l.slp_admm_batch_set_stop(st._h, *a))  # noqa: E731
        for bad in ((float("nan"), 1e-2, 1), (float("inf"), 1e-2, 1), (1e-2, float("nan"), 1), (1e-2, float("inf"), 1), (1e-2, -1e-3, 1),
                    (1e-2, 1e-2, 0), (1e-2, 1e-2, -4)):
            assert call(*bad) != 0, bad
            assert "tol_residual and tol_step must be finite and >= 0 with check_every >= 1" in _lib.last_error()
        st.iterate(3)
        st.sweep_step()
        with pytest.raises(SlpError, match="between sweep_step and multiplier_step"):
            st.set_stop(1e-2, 1e-2, 1)
        with pytest.raises(SlpError, match="between sweep_step and multiplier_step"):
            st.set_stop(None, None)
        st.multiplier_step()
        st.set_stop(1e-2, 1e-2, 1)
        assert call(-1.0, float("nan"), 0) == 0   # tol_residual < 0 turns the test off, whatever comes with it
        got = st.stop_state()
        assert np.array_equal(got[0], np.full(5, 4)) and not got[1].any()
    finally:
        st.close()
