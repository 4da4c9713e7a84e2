"""Host side of the per-instance stopping test of the batched ADMM solver (``lp_admm_batch_until``,
``SparseLP.solve_admm_batch_until``, ``ADMMBatchState.set_stop`` / ``stop_state``): the refusals come before the library is
touched, the new names and the two prototypes that include/slp_hip_ext.h brings along are there and bound, the batch restatement
(tests/admm_batch_stop_cpu.py) has one counter and sticky flags, and the fixture batches of tests/test_gpu_admm_batch_stop.py
have the spread of stopping iterations that makes them a test -- conditions on the inputs, derived from the restatement on the
oracle's iterates alone.  None of it needs a GPU."""
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest

import admm_batch_stop_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from pysparselp_amd import _lib, lp_admm_batch_until
from pysparselp_amd.ADMM import ADMMBatchState
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the CP form)
from test_gpu_admm_batch import _instances, _of_instance

sys.path.insert(0, os.path.join(REPO, "tools"))
import fuzz_batched  # noqa: E402

BATCH = 5
EVERY = 10
# name -> (fixture, what varies between the instances, (tol_residual, tol_step), iterations of the run)
BATCHES = {
    "potts8": ("potts8", ("c",), (1e-2, 1e-2), 300),
    "potts8_mixed": ("potts8", ("c",), (1e-3, 1e-3), 200),
    "sc105": ("sc105", ("c",), (1e-2, 1e-2), 300),
    "random1": ("random1", ("c", "bounds", "x0"), (1e-2, 1e-2), 300),
}


@functools.lru_cache(maxsize=None)
def batch_args(name, batch=BATCH):
    """The arguments of ``lp_admm_batch`` for a batch of ``BATCHES`` (shared, never modified)."""
    case, vary, _, _ = BATCHES[name]
    return _instances(load_golden("lp_" + case), batch, seed=len(case), vary=vary)


@functools.lru_cache(maxsize=None)
def batch_curves(name, batch=BATCH):
    """Per instance the restatement's ``(residual_t, step_t)`` over the run of the batch (shared, read only)."""
    return admm_batch_stop_cpu.batch_curves(batch_args(name, batch), BATCHES[name][3], _of_instance)


def batch_stops(name, batch=BATCH):
    """Per instance its stopping iteration under the restatement, ``None``: still running at the end of the run."""
    _, _, tol, total = BATCHES[name]
    return admm_batch_stop_cpu.stopping_iterations(batch_curves(name, batch), *tol, EVERY, total)


# the batch with an instance whose arithmetic overflows: the entry points refuse a cost or a start that is not finite, so the NaN
# has to arise in the iteration.  A cost of +-1e308 on a variable with an infinite bound that inequality rows meet, on the side of
# that bound, drives the variable to about 1e307 in the first sweep, the row sums to infinity in the next ones and inf - inf to NaN.
NAN_SEED, NAN_BATCH, NAN_INSTANCE, NAN_WITHIN = 5, 5, 2, 10   # instance 2: in the middle of the first tile of four
NAN_TOL, NAN_EVERY, NAN_TOTAL = (0.1, 0.1), (1, 3), 40       # generous: a record of 0.0 in place of a dropped NaN would stop at once


def _nan_candidate(rng):
    """A batch of ``NAN_BATCH`` over a ``random_lp(rng, "admm", 12)`` whose instance ``NAN_INSTANCE`` has the LP's own costs with
    +-1e308 on the first variable that has an infinite bound and an entry in an inequality row; None without such a variable."""
    lp = fuzz_batched.random_lp(rng, "admm", 12)
    met = np.diff(lp["a_ineq"].tocsc().indptr) > 0
    free = [j for j in range(12) if met[j] and (np.isinf(lp["ub"][j]) or np.isinf(lp["lb"][j]))]
    if not free:
        return None
    args = fuzz_batched.batch_of(rng, lp, NAN_BATCH, "admm")
    args["cs"] = args.pop("c")
    args["cs"][NAN_INSTANCE] = lp["c"]
    args["cs"][NAN_INSTANCE, free[0]] = -1e308 if np.isinf(lp["ub"][free[0]]) else 1e308
    return args


def _nan_condition(curves):
    """The NaN instance's residual and step are NaN from some iteration within ``NAN_WITHIN`` on, its batch-mates' stay finite."""
    mates = all(np.all(np.isfinite(c)) for k, pair in enumerate(curves) if k != NAN_INSTANCE for c in pair)
    bad = [np.isnan(c) for c in curves[NAN_INSTANCE]]
    return mates and all(b[NAN_WITHIN - 1:].all() for b in bad)


@functools.lru_cache(maxsize=None)
def nan_batch():
    """``(args, curves over NAN_TOTAL iterations)`` of the first of twelve draws of ``RandomState(NAN_SEED)`` that meets
    ``_nan_condition`` (shared, never modified)."""
    rng = np.random.RandomState(NAN_SEED)
    for _ in range(12):
        args = _nan_candidate(rng)
        if args is None:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            curves = admm_batch_stop_cpu.batch_curves(args, NAN_TOTAL, _of_instance)
        if _nan_condition(curves):
            return args, curves
    raise AssertionError("no draw overflows")


class _NoState(ADMMBatchState):
    """A state without a device: ``set_stop`` must refuse before it looks for one."""

    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


def _call(name, *stop, **kw):
    a = batch_args(name)
    return lp_admm_batch_until(a["cs"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"], *stop, x0=a["x0"],
                               **kw)


def _lp():
    return lp_from_golden(load_golden("lp_potts8"), SparseLP)


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    lp, st = _lp(), _NoState()
    costs = np.tile(lp.costsvector, (2, 1))
    for tol in BAD_TOL:
        for name, stop in (("tol_residual", (tol, 1e-2)), ("tol_step", (1e-2, tol))):
            match = f"^{name} must be a finite float >= 0"
            with pytest.raises(ValueError, match=match):
                _call("potts8", *stop)
            with pytest.raises(ValueError, match=match):
                lp.solve_admm_batch_until(costs, *stop)
            if not (name == "tol_residual" and tol is None):   # None is how the state's test is turned off
                with pytest.raises(ValueError, match=match):
                    st.set_stop(*stop)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            _call("potts8", 1e-2, 1e-2, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            lp.solve_admm_batch_until(costs, 1e-2, 1e-2, check_every=every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            st.set_stop(1e-2, 1e-2, every)
    # the checks of the batch itself stay those of lp_admm_batch / solve_admm_batch
    a = batch_args("potts8")
    with pytest.raises(ValueError):
        lp_admm_batch_until(a["cs"][0], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"], 1e-2, 1e-2)
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_admm_batch_until(costs[:, :-1], 1e-2, 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        _call("potts8", 0.0, 0, 1, nb_iter=3)
    lp = _lp()
    with pytest.raises(AssertionError, match="library was loaded"):
        lp.solve_admm_batch_until(np.tile(lp.costsvector, (2, 1)), 1e-2, np.float32(0.5), nb_iter=3)


def test_names_and_signatures():
    assert "lp_admm_batch_until" in pysparselp_amd.__all__ and "ADMMBatchState" in pysparselp_amd.__all__
    assert pysparselp_amd.lp_admm_batch_until is pysparselp_amd.ADMM.lp_admm_batch_until
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert all(hasattr(pysparselp_amd, name) for name in pysparselp_amd.__all__)
    assert "lp_admm_batch_until" in pysparselp_amd.__doc__ and "solve_admm_batch_until" in pysparselp_amd.__doc__
    assert str(inspect.signature(pysparselp_amd.lp_admm_batch_until)) == (
        "(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_residual, tol_step, check_every=10, x0=None, gamma_eq=2, gamma_ineq=3, "
        "nb_iter=10000, callback_func=None, max_time=None, use_preconditioning=True, nb_iter_plot=10)")
    assert str(inspect.signature(SparseLP.solve_admm_batch_until)) == (
        "(self, costs, tol_residual, tol_step, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10, "
        "ground_truth=None, ground_truth_indices=None)")
    assert str(inspect.signature(ADMMBatchState.set_stop)) == "(self, tol_residual, tol_step, check_every=1)"
    assert str(inspect.signature(ADMMBatchState.stop_state)) == "(self)"
    for doc in (ADMMBatchState.set_stop.__doc__, ADMMBatchState.stop_state.__doc__):
        assert "for the life of the state" in " ".join(doc.split())   # the one difference from the list solver
    # lp_admm_batch keeps its signature
    assert str(inspect.signature(pysparselp_amd.lp_admm_batch)) == (
        "(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, x0=None, gamma_eq=2, gamma_ineq=3, nb_iter=100, callback_func=None, "
        "max_time=None, use_preconditioning=True, nb_iter_plot=10)")


def test_the_two_prototypes_are_in_the_extension_header_and_bound():
    strip = lambda text: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))  # noqa: E731
    # slp_hip_ext.h declares them through a header of their own, which it includes: its own text keeps its two declarations
    assert '#include "slp_hip_ext_admm_batch.h"' in open(os.path.join(REPO, "include", "slp_hip_ext.h")).read()
    ext = strip(open(os.path.join(REPO, "include", "slp_hip_ext_admm_batch.h")).read())
    assert "int slp_admm_batch_set_stop(slp_admm_batch *s, double tol_residual, double tol_step, int64_t check_every);" in ext
    assert ("int slp_admm_batch_stop_state(slp_admm_batch *s, int64_t *iterations, int32_t *stopped, double *residual, double *step);"
            in ext)
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    new = list(_lib.EXT_ADMM_BATCH_SYMBOLS)
    assert declared == sorted(new) == ["slp_admm_batch_set_stop", "slp_admm_batch_stop_state"]
    assert _lib.EXT_ADMM_BATCH_SYMBOLS == tuple(_lib._EXT_ADMM_BATCH_SIGNATURES)
    base = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    lib = _lib.load()   # dlopen works without a GPU
    for name in new:
        assert name not in base and name not in _lib.EXPORTED_SYMBOLS and name not in _lib.EXT_SYMBOLS and hasattr(lib, name), name
    assert lib.slp_admm_batch_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_admm_batch_stop_state.argtypes == [_lib.c_vp] * 5
    assert lib.slp_admm_batch_set_stop.restype is _lib.c_int and lib.slp_admm_batch_stop_state.restype is _lib.c_int
    assert len(_lib.EXPORTED_SYMBOLS) == 215   # include/slp_hip.h stays as it is
    readme = open(os.path.join(REPO, "README.md")).read()
    assert all(name in readme for name in new) and "lp_admm_batch_until" in readme


def test_the_restatement_on_hand_made_curves():
    inf, nan = np.inf, np.nan
    # iteration:            1    2    3     4    5     6
    a = (np.array([4.0, 0.25, 1.0, 0.0, 0.0, 0.0]), np.array([2.0, 0.5, 0.0, 0.0, 0.0, 0.0]))    # meets (0.25, 0.5) at 2
    b = (np.array([4.0, 4.0, 4.0, 0.5, 0.125, 0.125]), np.array([2.0, 2.0, 2.0, 0.5, 0.5, 0.25]))  # meets it at 5 only
    c = (np.array([nan, 0.0, 0.0, 0.0, 0.0, 0.0]), np.array([0.0, nan, nan, nan, nan, nan]))      # a NaN stays
    curves = (a, b, c)
    state = functools.partial(admm_batch_stop_cpu.stop_state, curves)

    def same(got, iterations, stopped, residual, step):
        assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == got[3].dtype == np.float64
        assert np.array_equal(got[0], iterations) and np.array_equal(got[1], stopped), got
        assert np.array_equal(got[2], residual, equal_nan=True) and np.array_equal(got[3], step, equal_nan=True), got

    # one counter: the running instances report the state's t, a stopped one its own; a NaN never stops, whatever the tolerance
    same(state((0.25, 0.5, 1), 4), [2, 4, 4], [True, False, False], [0.25, 0.5, 0.0], [0.5, 0.5, nan])
    same(state((0.25, 0.5, 1), 6), [2, 5, 6], [True, True, False], [0.25, 0.125, 0.0], [0.5, 0.5, nan])
    same(state((1e300, 1e300, 1), 1), [1, 1, 1], [True, True, False], [4.0, 4.0, nan], [2.0, 2.0, 0.0])
    # +inf before the first check, for every instance
    same(state((0.25, 0.5, 4), 3), [3, 3, 3], [False] * 3, [inf] * 3, [inf] * 3)
    same(state([(2, 0.25, 0.5, 1)], 2), [2, 2, 2], [False] * 3, [inf] * 3, [inf] * 3)   # armed when two iterations are complete
    # sticky: instance 0 stopped at 2; re-armed at 3 with tolerances it never meets again it stays stopped at 2 with its record,
    # while instance 1 now runs under the tighter ones
    same(state([(0, 0.25, 0.5, 1), (3, 0.0, 0.0, 1)], 6), [2, 6, 6], [True, False, False], [0.25, 0.125, 0.0], [0.5, 0.25, nan])
    # ... and a re-arm with looser ones stops instance 1 at the next check, not instance 0 again
    same(state([(0, 0.25, 0.5, 1), (3, 0.5, 0.5, 2)], 6), [2, 4, 6], [True, True, False], [0.25, 0.5, 0.0], [0.5, 0.5, nan])
    # turning off keeps the flags and the last evaluated numbers; the running instances go on untested
    same(state([(0, 0.25, 0.5, 1), (3, None, None, 1)], 6), [2, 6, 6], [True, False, False], [0.25, 4.0, 0.0], [0.5, 2.0, nan])
    # off and on again: the count went on while the test was off
    same(state([(0, 0.25, 0.5, 1), (3, None, None, 1), (5, 0.25, 0.5, 1)], 6), [2, 6, 6], [True, True, False], [0.25, 0.125, 0.0],
         [0.5, 0.25, nan])
    assert admm_batch_stop_cpu.stopping_iterations(curves, 0.25, 0.5, 1, 6) == [2, 5, None]
    assert admm_batch_stop_cpu.stopping_iterations(curves, 0.25, 0.5, 1, 4) == [2, None, None]


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_fixture_batches_keep_their_spread(name):
    """What makes the GPU cases a test, recomputed from the restatement on the oracle's iterates: every batch shows at least two
    distinct stopping iterations, all of them check iterations inside the run, and the mixed batch has stopped and running
    instances side by side."""
    stops = batch_stops(name)
    total = BATCHES[name][3]
    reached = [t for t in stops if t is not None]
    print(name, stops)
    assert len(stops) == BATCH and len(set(reached)) >= 2, stops
    assert all(t % EVERY == 0 and EVERY <= t < total for t in reached), stops
    if name == "potts8_mixed":
        assert 1 <= len(reached) < BATCH, stops
    else:
        assert len(reached) == BATCH, stops
    if name == "sc105":   # with a tile of four: instance 1 stops long before its tile-mates 0, 2, 3
        assert stops[1] + 2 * EVERY <= max(stops[0], stops[2], stops[3]), stops
    # either tolerance alone stops an instance no later than both together
    _, _, tol, _ = BATCHES[name]
    loose_r = admm_batch_stop_cpu.stopping_iterations(batch_curves(name), 1e300, tol[1], EVERY, total)
    loose_s = admm_batch_stop_cpu.stopping_iterations(batch_curves(name), tol[0], 1e300, EVERY, total)
    for k, t in enumerate(stops):
        if t is not None:
            assert loose_r[k] <= t and loose_s[k] <= t


def test_a_reordered_batch_has_a_tile_that_stops_long_before_the_other():
    """The workgroup's early return needs a whole tile of four that is stopped while another still runs: the sc105 batch of eight
    has four instances that stop at least two checks before the last one of the others."""
    name = "sc105"
    stops = admm_batch_stop_cpu.stopping_iterations(batch_curves(name, 8), *BATCHES[name][2], EVERY, BATCHES[name][3])
    assert all(t is not None for t in stops), stops
    order = np.argsort(stops, kind="stable")
    assert stops[order[3]] + 2 * EVERY <= stops[order[-1]], stops


def test_the_nan_batch_overflows_in_one_instance_only():
    """What makes the GPU case a test: the seeded search finds a batch whose instance ``NAN_INSTANCE`` -- in the middle of a tile of
    four -- has NaN curves within ``NAN_WITHIN`` iterations, after at least one finite check, while its four batch-mates stay finite
    and all stop under ``NAN_TOL`` at either cadence, not all at one iteration.  The restatement never stops the NaN instance and
    keeps the NaN in its record."""
    args, curves = nan_batch()
    assert args["cs"].shape == (NAN_BATCH, 12) and np.all(np.isfinite(args["cs"])) and np.abs(args["cs"][NAN_INSTANCE]).max() == 1e308
    assert _nan_condition(curves) and NAN_INSTANCE % 4 in (1, 2) and NAN_INSTANCE < 4 < NAN_BATCH
    residual, step = curves[NAN_INSTANCE]
    first = int(np.argmax(np.isnan(residual) | np.isnan(step))) + 1
    print("the NaN instance:", residual[:first], step[:first], "NaN from iteration", first)
    assert 2 <= first <= NAN_WITHIN and np.all(np.isnan(residual[first - 1:])) and np.all(np.isnan(step[first - 1:]))
    for every in NAN_EVERY:
        stops = admm_batch_stop_cpu.stopping_iterations(curves, *NAN_TOL, every, NAN_TOTAL)
        print("every", every, "stops", stops)
        assert stops[NAN_INSTANCE] is None and all(t is not None for k, t in enumerate(stops) if k != NAN_INSTANCE), stops
        assert len({t for t in stops if t is not None}) >= 2 and min(t for t in stops if t is not None) > first
        want = admm_batch_stop_cpu.stop_state(curves, NAN_TOL + (every,), NAN_TOTAL)
        assert want[0][NAN_INSTANCE] == NAN_TOTAL and not want[1][NAN_INSTANCE]
        assert np.isnan(want[2][NAN_INSTANCE]) and np.isnan(want[3][NAN_INSTANCE])
