"""Host side of the per-LP stopping test of the ADMM list solver (``lp_admm_many_until``, ``solve_admm_many_until``,
``ADMMManyState.set_stop`` / ``stop_state``): the refusals come before the library is touched, the new names and prototypes are
there, and the fixture list of tests/test_gpu_admm_many_stop.py has the spread of stopping iterations that makes it a test -- a
condition on the inputs, derived from the numpy restatement (tests/admm_stop_cpu.py) alone.  None of it needs a GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import admm_stop_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden, solver_args
from pysparselp_amd import _lib, _many, lp_admm_many_until, solve_admm_many_until
from pysparselp_amd.ADMM import ADMMManyState
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the CP form)

CASES = ("sc50a", "sc105", "potts8", "random0", "random1", "random2")
ITERATIONS = 200


@functools.lru_cache(maxsize=None)
def fixture_curves(case, nb_iter=ITERATIONS):
    """``(residual_t, step_t)``, ``t = 1 .. nb_iter``, of a golden LP on the restatement (shared, never modified)."""
    curves = admm_stop_cpu.oracle_curves(solver_args(load_golden("lp_" + case)), nb_iter)
    for c in curves:
        c.setflags(write=False)
    return curves


def stops(tol_residual, tol_step, every, cases=CASES):
    return {c: admm_stop_cpu.stopping_iteration(*fixture_curves(c), tol_residual, tol_step, every) for c in cases}


def _problems(cases=("random1", "sc50a")):
    return [solver_args(load_golden("lp_" + c)) for c in cases]


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    ps = _problems()
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    for tol in BAD_TOL:
        with pytest.raises(ValueError, match="tol_residual must be a finite float >= 0"):
            lp_admm_many_until(ps, tol, 1e-2)
        with pytest.raises(ValueError, match="tol_step must be a finite float >= 0"):
            lp_admm_many_until(ps, 1e-2, tol)
        with pytest.raises(ValueError, match="tol_residual must be a finite float >= 0"):
            solve_admm_many_until(lps, tol, 1e-2)
        with pytest.raises(ValueError, match="tol_step must be a finite float >= 0"):
            solve_admm_many_until(lps, 1e-2, tol)
        with pytest.raises(ValueError, match="^tol_step must be a finite float >= 0"):
            _many.check_stop(tol, 1, "tol_step")
        with pytest.raises(ValueError, match="^tol must be a finite float >= 0"):   # the Chambolle-Pock callers' message
            _many.check_stop(tol, 1)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            lp_admm_many_until(ps, 1e-2, 1e-2, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            solve_admm_many_until(lps, 1e-2, 1e-2, check_every=every)
    assert _many.check_stop(0, np.int64(3), "tol_residual") == (0.0, 3)
    # the checks of the list itself stay those of lp_admm_many
    with pytest.raises(ValueError, match="empty list"):
        lp_admm_many_until([], 1e-2, 1e-2)
    with pytest.raises(ValueError, match="LP 1 is not a tuple of 8"):
        lp_admm_many_until([ps[0], ps[1][:7]], 1e-2, 1e-2)
    with pytest.raises(ValueError, match="empty list"):
        solve_admm_many_until([], 1e-2, 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_admm_many_until(_problems(), 0.0, 0, 1, nb_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_admm_many_until([lp_from_golden(load_golden("lp_potts8"), SparseLP)], 1e-2, np.float32(0.5), nb_iter=3)


def test_the_stop_info_carries_the_residual_only_when_asked():
    info = _many.new_stop_info(4, [1, 3], residual=True)
    assert sorted(info) == ["iterations", "residual", "step", "stopped"]
    assert info["iterations"].dtype == np.int64 and info["stopped"].dtype == bool
    assert info["residual"].dtype == np.float64 and info["step"].dtype == np.float64
    assert np.array_equal(info["stopped"], [True, False, True, False])
    assert np.array_equal(info["residual"], [0.0, np.inf, 0.0, np.inf]) and np.array_equal(info["step"], info["residual"])
    held = dict(info)
    _many.spread_stop_state(info, [1, 3], (np.array([7, 20]), np.array([True, False]), np.array([1e-3, 0.5]), np.array([2e-3, 0.25])))
    assert np.array_equal(held["iterations"], [0, 7, 0, 20]) and np.array_equal(held["stopped"], [True, True, True, False])
    assert np.array_equal(held["residual"], [0.0, 1e-3, 0.0, 0.5]) and np.array_equal(held["step"], [0.0, 2e-3, 0.0, 0.25])
    # what the Chambolle-Pock callers get is what they got
    info = _many.new_stop_info(3, [0])
    assert sorted(info) == ["iterations", "step", "stopped"] and np.array_equal(info["step"], [np.inf, 0.0, 0.0])
    _many.spread_stop_state(info, [0], (np.array([5]), np.array([True]), np.array([0.125])))
    assert info["iterations"][0] == 5 and info["stopped"].all() and info["step"][0] == 0.125


def test_names_and_signatures():
    for name in ("lp_admm_many_until", "solve_admm_many_until", "ADMMManyState"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name), name
    assert str(inspect.signature(lp_admm_many_until)) == (
        "(problems, tol_residual, tol_step, check_every=10, x0=None, gamma_eq=2, gamma_ineq=3, nb_iter=10000, callback_func=None, "
        "max_time=None, use_preconditioning=True, nb_iter_plot=10)")
    assert str(inspect.signature(solve_admm_many_until)) == (
        "(lps, tol_residual, tol_step, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10)")
    assert pysparselp_amd.SparseLP.solve_admm_many_until is solve_admm_many_until
    assert str(inspect.signature(ADMMManyState.set_stop)) == "(self, tol_residual, tol_step, check_every=1)"
    assert str(inspect.signature(ADMMManyState.stop_state)) == "(self)"


def test_the_two_prototypes_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert "int slp_many_admm_set_stop(slp_admm_many *s, double tol_residual, double tol_step, int64_t check_every);" in text
    assert ("int slp_many_admm_stop_state(slp_admm_many *s, int64_t *iterations, int32_t *stopped, double *residual, double *step);"
            in text)
    new = sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_many_admm_"))
    assert new == ["slp_many_admm_set_stop", "slp_many_admm_stop_state"]
    lib = _lib.load()   # dlopen works without a GPU
    for name in new:
        assert hasattr(lib, name), name
    assert lib.slp_many_admm_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_many_admm_stop_state.argtypes == [_lib.c_vp] * 5
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"C ABI ({len(_lib.EXPORTED_SYMBOLS)} entry points)" in readme


def test_the_restatement_on_hand_made_iterates():
    xs = [np.array([0.0, 0.0]), np.array([1.0, -2.0]), np.array([1.0, -2.5]), np.array([1.0, -2.5]), np.array([1.0, -2.5])]
    residual, step = admm_stop_cpu.curves_of(xs, [4.0, 0.25, 1.0, 0.0])
    assert np.array_equal(step, [2.0, 0.5, 0.0, 0.0]) and np.array_equal(residual, [4.0, 0.25, 1.0, 0.0])
    at = functools.partial(admm_stop_cpu.stopping_iteration, residual, step)
    assert at(0.25, 0.5, 1) == 2
    assert at(0.25, 0.25, 1) == 4          # iteration 2 meets the residual only, iteration 3 the step only
    assert at(0.25, 0.5, 3) is None        # iteration 3 is the only check: its residual is 1.0
    assert at(0.25, 0.5, 4) == 4
    assert at(0.0, 0.0, 1) == 4            # an exact fixed point with an exact residual
    assert at(0.25, 0.5, 1, after=2) == 4  # re-armed after iteration 2
    assert at(10.0, 0.0, 1) == 3 and at(0.0, 10.0, 1) == 4   # the two tolerances act on their own
    state = functools.partial(admm_stop_cpu.stop_state, residual, step)
    assert state(0.25, 0.5, 3, 4) == (4, False, 1.0, 0.0)
    assert state(0.25, 0.5, 1, 4) == (2, True, 0.25, 0.5)
    assert state(0.1, 0.1, 3, 2) == (2, False, np.inf, np.inf)
    assert state(0.1, 0.1, 3, 2, after=1, before=(0.5, 0.75)) == (2, False, 0.5, 0.75)
    # a NaN in an iterate makes the steps on both sides of it a NaN, as np.max does: never a stop
    xs[2] = np.array([1.0, np.nan])
    residual, step = admm_stop_cpu.curves_of(xs, [4.0, np.nan, 1.0, 0.0])
    assert np.isnan(step[1]) and np.isnan(step[2]) and step[3] == 0.0 and np.isnan(residual[1])
    assert admm_stop_cpu.stopping_iteration(residual[:3], step[:3], 1e9, 1e9, 1, after=1) is None
    # no row: the residual is 0.0
    from oracle import oracle
    assert admm_stop_cpu.residual_of(oracle.Csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (0, 2)),
                                     np.zeros(0), np.ones(2)) == 0.0


def test_the_fixture_list_spreads_its_stopping_iterations():
    """What makes the GPU cases a test, recomputed from the restatement on the oracle's iterates."""
    # 1e-3 / 1e-3: exactly three LPs stop, at pairwise distinct iterations inside the run; the cadence moves two of them
    by_every = {every: stops(1e-3, 1e-3, every) for every in (1, 4, 10)}
    for every, got in by_every.items():
        reached = {c: t for c, t in got.items() if t is not None}
        assert sorted(reached) == ["potts8", "random1", "random2"], got
        assert len(set(reached.values())) == 3 and all(1 < t < ITERATIONS and t % every == 0 for t in reached.values()), got
    assert by_every[1]["potts8"] == by_every[4]["potts8"] == by_every[10]["potts8"]
    for c in ("random1", "random2"):
        assert by_every[1][c] < by_every[10][c] and by_every[1][c] <= by_every[4][c] <= by_every[10][c]
    # 1e-2 / 1e-2: all six stop; a coarser cadence moves some later
    fine = stops(1e-2, 1e-2, 1)
    assert all(t is not None and 1 < t < ITERATIONS for t in fine.values()) and len(set(fine.values())) == 6, fine
    for every in (4, 10):
        later = stops(1e-2, 1e-2, every)
        assert all(later[c] is not None and later[c] % every == 0 and later[c] >= fine[c] for c in CASES), later
        assert any(later[c] > fine[c] for c in CASES)
    # the two tolerances act independently
    assert 1 < stops(1e-1, 1e-3, 1)["random0"] < 100 and stops(1e-3, 1e-1, 1)["random0"] is None
    # tol = 0: nobody stops (potts8 comes close to a fixed point and does not reach one)
    assert all(t is None for t in stops(0.0, 0.0, 1).values())
    residual, step = fixture_curves("potts8")
    assert 0.0 < residual.min() and 0.0 < step.min() < 1e-6
