"""Host side of the per-LP stopping test of the Chambolle-Pock list solver (``chambolle_pock_ppd_many_until``,
``solve_many_until``, ``CPManyState.set_stop`` / ``stop_state``): the refusals come before the library is touched, the new names
and prototypes are there, and the fixture list of tests/test_gpu_cp_many_stop.py has the spread of stopping iterations that makes
it a test -- a condition on the inputs, derived from the numpy restatement (tests/cp_stop_cpu.py) alone.  None of it needs a GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

import cp_stop_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from pysparselp_amd import _lib, _many, chambolle_pock_ppd_many_until, solve_many_until
from pysparselp_amd.ChambollePockPPD import CPManyState
from pysparselp_amd.SparseLP import SparseLP
from test_oracle_golden import _reduced

CASES = ("potts8", "sc50a", "sc105", "random0", "random1", "random2")
ITERATIONS = 200


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load or bind the library fails the test: validation must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


@functools.lru_cache(maxsize=None)
def fixture_steps(case, nb_iter=ITERATIONS):
    """``step_t``, ``t = 1 .. nb_iter``, of a reduced golden LP on the restatement (shared, never modified)."""
    steps = cp_stop_cpu.steps_of(*cp_stop_cpu.oracle_iterates(_reduced(load_golden("lp_" + case)), nb_iter))
    steps.setflags(write=False)
    return steps


def _problems(cases=("random1", "sc50a")):
    return [_reduced(load_golden("lp_" + c)) for c in cases]


BAD_TOL = (-1e-3, float("nan"), float("inf"), None, "1e-2", True, 1j)
BAD_EVERY = (0, -3, 2.0, 1.5, None, "4", True)


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):
    ps = _problems()
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    for tol in BAD_TOL:
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            chambolle_pock_ppd_many_until(ps, tol)
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            solve_many_until(lps, tol)
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            _many.check_stop(tol, 1)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            chambolle_pock_ppd_many_until(ps, 1e-2, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            solve_many_until(lps, 1e-2, check_every=every)
    assert _many.check_stop(0, np.int64(3)) == (0.0, 3) and _many.check_stop(np.float32(0.5), 1) == (0.5, 1)
    # the checks of the list itself stay those of chambolle_pock_ppd_many
    with pytest.raises(ValueError, match="empty list"):
        chambolle_pock_ppd_many_until([], 1e-2)
    with pytest.raises(ValueError, match="LP 1 is not a tuple of 8"):
        chambolle_pock_ppd_many_until([ps[0], ps[1][:7]], 1e-2)
    with pytest.raises(ValueError, match="empty list"):
        solve_many_until([], 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):
    with pytest.raises(AssertionError, match="library was loaded"):
        chambolle_pock_ppd_many_until(_problems(), 0.0, 1, nb_max_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_many_until([lp_from_golden(load_golden("lp_potts8"), SparseLP)], 1e-2, nb_iter=3)


def test_lps_without_rows_are_stopped_after_no_iteration(no_library):
    rng = np.random.RandomState(5)
    ps = []
    for n in (4, 1):
        c = rng.randn(n)
        ps.append((c, None, None, scipy.sparse.csr_matrix((0, n)), None, np.zeros(0), -rng.rand(n) - 1, rng.rand(n) + 1))
    xs, best, info = chambolle_pock_ppd_many_until(ps, 1e-2)
    assert best == [None, None]
    for (c, *_, lb, ub), x in zip(ps, xs):
        assert np.array_equal(x, np.where(c > 0, lb, np.where(c < 0, ub, 0.0)))
    assert sorted(info) == ["iterations", "step", "stopped"]
    assert info["iterations"].dtype == np.int64 and info["stopped"].dtype == bool and info["step"].dtype == np.float64
    assert np.array_equal(info["iterations"], [0, 0]) and np.array_equal(info["stopped"], [True, True])
    assert np.array_equal(info["step"], [0.0, 0.0])


def test_the_stop_state_is_spread_over_the_lps_that_took_no_part():
    info = _many.new_stop_info(5, [1, 3, 4])
    assert np.array_equal(info["stopped"], [True, False, True, False, False])
    assert np.array_equal(info["step"], [0.0, np.inf, 0.0, np.inf, np.inf]) and not info["iterations"].any()
    held = dict(info)
    _many.spread_stop_state(info, [1, 3, 4], (np.array([7, 20, 13]), np.array([True, False, True]), np.array([1e-3, 0.5, 0.0])))
    assert np.array_equal(held["iterations"], [0, 7, 0, 20, 13])   # in place: the arrays a callback holds are current
    assert np.array_equal(held["stopped"], [True, True, True, False, True])
    assert np.array_equal(held["step"], [0.0, 1e-3, 0.0, 0.5, 0.0])


def test_names_and_signatures():
    for name in ("chambolle_pock_ppd_many_until", "solve_many_until", "CPManyState"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name), name
    assert str(inspect.signature(chambolle_pock_ppd_many_until)) == (
        "(problems, tol, check_every=10, x0=None, alpha=1, theta=1, nb_max_iter=10000, callback_func=None, max_time=None, nb_iter_plot=10)")
    assert str(inspect.signature(solve_many_until)) == (
        "(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10)")
    assert pysparselp_amd.SparseLP.solve_many_until is solve_many_until
    assert str(inspect.signature(CPManyState.set_stop)) == "(self, tol, check_every=1)"
    assert str(inspect.signature(CPManyState.stop_state)) == "(self)"


def test_the_two_prototypes_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert "int slp_many_cp_set_stop(slp_cp_many *s, double tol, int64_t check_every);" in text
    assert "int slp_many_cp_stop_state(slp_cp_many *s, int64_t *iterations, int32_t *stopped, double *step);" in text
    new = sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_many_cp_"))
    assert new == ["slp_many_cp_set_stop", "slp_many_cp_stop_state"]
    lib = _lib.load()   # dlopen works without a GPU
    for name in new:
        assert hasattr(lib, name), name
    assert lib.slp_many_cp_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_many_cp_stop_state.argtypes == [_lib.c_vp] * 4
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"C ABI ({len(_lib.EXPORTED_SYMBOLS)} entry points)" in readme


def test_the_restatement_on_hand_made_iterates():
    xs = [np.array([0.0, 0.0]), np.array([1.0, -2.0]), np.array([1.0, -2.5]), np.array([1.0, -2.5]), np.array([1.0, -2.5])]
    ys = [np.array([0.0]), np.array([0.25]), np.array([0.25]), np.array([1.0]), np.array([1.0])]
    steps = cp_stop_cpu.steps_of(xs, ys)
    assert np.array_equal(steps, [2.0, 0.5, 0.75, 0.0])
    assert cp_stop_cpu.stopping_iteration(steps, 0.5, 1) == 2
    assert cp_stop_cpu.stopping_iteration(steps, 0.5, 3) is None       # iteration 3 is the only check: 0.75
    assert cp_stop_cpu.stopping_iteration(steps, 0.5, 4) == 4
    assert cp_stop_cpu.stopping_iteration(steps, 0.0, 1) == 4           # an exact fixed point
    assert cp_stop_cpu.stopping_iteration(steps, 0.5, 1, after=2) == 4  # re-armed after iteration 2
    assert cp_stop_cpu.stop_state(steps, 0.5, 3, 4) == (4, False, 0.75)
    assert cp_stop_cpu.stop_state(steps, 0.5, 1, 4) == (2, True, 0.5)
    assert cp_stop_cpu.stop_state(steps, 0.1, 3, 2) == (2, False, np.inf)
    ys[2] = np.array([np.nan])   # a NaN among the differences makes the step a NaN, as np.max does: never a stop
    steps = cp_stop_cpu.steps_of(xs, ys)
    assert np.isnan(steps[1]) and np.isnan(steps[2]) and steps[3] == 0.0
    assert cp_stop_cpu.stopping_iteration(steps[:3], 1e9, 1, after=1) is None


def test_the_fixture_list_spreads_its_stopping_iterations():
    """What makes the GPU cases a test: at ``tol = 1e-2, check_every = 1`` at least four LPs of the list stop at pairwise distinct
    iterations inside the run, and sc50a does not stop at all."""
    stops = {c: cp_stop_cpu.stopping_iteration(fixture_steps(c), 1e-2, 1) for c in CASES}
    assert stops["sc50a"] is None
    reached = [t for t in stops.values() if t is not None]
    assert len(set(reached)) >= 4 and len(reached) == 5, stops
    assert all(1 < t < ITERATIONS for t in reached), stops
    # the cadence matters: a coarser one moves a stop to a later check iteration
    for every in (4, 10):
        later = {c: cp_stop_cpu.stopping_iteration(fixture_steps(c), 1e-2, every) for c in CASES}
        assert later["sc50a"] is None
        assert all(later[c] is not None and later[c] % every == 0 and later[c] >= stops[c] for c in CASES if c != "sc50a"), later
        assert any(later[c] > stops[c] for c in CASES if c != "sc50a")
    # potts8 reaches an exact fixed point
    t = cp_stop_cpu.stopping_iteration(fixture_steps("potts8"), 0.0, 1)
    assert t is not None and fixture_steps("potts8")[t - 1] == 0.0
