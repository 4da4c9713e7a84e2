"""Host side of the per-LP stopping test of dual gradient ascent on a list (``dual_gradient_ascent_many_until``,
``solve_dga_many_until``, ``DeviceDGAMany.set_stop`` / ``stop_state``): the numpy restatement (tests/dga_stop_cpu.py) on the fifteen
small LPs of tests/dga_many_cases.py gives the recorded stopping iterations in both orders of sums, the refusals come before the
library is touched, the new names and prototypes are there, and the window of tie draws goes on without a stopped reader (a
stand-alone program under AddressSanitizer and UBSan, run as a child process).  None of it needs a GPU."""
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dga_stop_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from dga_many_cases import LP, extra_list, mixed_list
from pysparselp_amd import _lib, _many, dual_gradient_ascent_many_until, solve_dga_many_until
from pysparselp_amd.DualGradientAscent import DeviceDGAMany
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401

ITERATIONS = 130
TOL = 1e-2
# the stopping iterations at tol = 1e-2, check_every = 10, LP by LP
STOPS_AT_10 = (10, 40, 30, 20, 20, 60, 30, 30, 10, 10, 50, 20, 20, 20, 10)
FIXED_POINTS = {5: 122, 8: 96}   # list index -> first iteration with step 0.0 (random0 with cost 5, potts8 with cost 2)


def fifteen():
    """The fifteen small LPs as ``dga_cpu`` takes them: the mixed list, then sc105, equalities_only, inequalities_only."""
    return [args for _, _, args in mixed_list()] + [args for _, args in extra_list()[:3]]


@functools.lru_cache(maxsize=None)
def fifteen_states(order="reference"):
    """Per LP ``dga_cpu``'s states after 0 .. ITERATIONS iterations (keys -1 .. ITERATIONS - 1); shared, never modified."""
    return tuple(dga_stop_cpu.states_of(args, ITERATIONS, order) for args in fifteen())


@functools.lru_cache(maxsize=None)
def fifteen_steps(order="reference"):
    """Per LP ``step_t``, ``t = 1 .. ITERATIONS``; shared, read-only."""
    out = tuple(dga_stop_cpu.steps_of(s) for s in fifteen_states(order))
    for steps in out:
        steps.setflags(write=False)
    return out


def expected(tol, every, total, steps=None):
    """``(iterations, stopped, step)`` of the restatement for the fifteen LPs."""
    steps = fifteen_steps() if steps is None else steps
    rows = [dga_stop_cpu.stop_state(s, tol, every, total) for s in steps]
    return tuple(np.array(col) for col in zip(*rows))


def test_the_restatement_reproduces_the_recorded_stopping_iterations():
    steps = fifteen_steps()
    assert len(steps) == 15 and all(s.shape == (ITERATIONS,) for s in steps)
    stops = tuple(dga_stop_cpu.stopping_iteration(s, TOL, 10) for s in steps)
    assert stops == STOPS_AT_10
    finer = [dga_stop_cpu.stopping_iteration(s, 1e-3, 10) for s in steps]
    assert all(t is not None and 10 <= t <= 100 and t % 10 == 0 for t in finer), finer
    assert min(finer) == 10 and max(finer) == 100
    # exact fixed points: two LPs, and only those, reach step 0.0 -- and stay there
    zero = {k: dga_stop_cpu.stopping_iteration(s, 0.0, 1) for k, s in enumerate(steps)}
    assert {k: t for k, t in zero.items() if t is not None} == FIXED_POINTS
    for k, t in FIXED_POINTS.items():
        assert not steps[k][t - 1:].any() and steps[k][t - 2] > 0.0
    # the step is not monotone, so the cadence matters: random1 with cost 2 falls to 1.9e-4 and stands at 1.9e-3 in the end
    k = 2
    assert mixed_list()[k][:2] == ("random1", 2)
    assert 1.8e-4 < steps[k].min() < 2.0e-4 and 1.8e-3 < steps[k][-1] < 2.0e-3
    every1 = [dga_stop_cpu.stopping_iteration(s, TOL, 1) for s in steps]
    assert all(a <= b for a, b in zip(every1, STOPS_AT_10)) and any(a < b - 9 for a, b in zip(every1, STOPS_AT_10))


def test_both_orders_of_sums_give_the_same_steps():
    for k, (ref, dev) in enumerate(zip(fifteen_steps("reference"), fifteen_steps("device"))):
        assert np.array_equal(ref, dev), k


def test_the_restatement_on_hand_made_states():
    def st(y_eq, y_ineq):
        return (None, np.array(y_eq, dtype=np.float64), None if y_ineq is None else np.array(y_ineq, dtype=np.float64), 0)

    states = {-1: st([0.0, 1.0], [2.0]), 0: st([0.5, 1.0], [2.0]), 1: st([0.5, 1.0], [0.0]), 2: st([0.5, 1.25], [0.0]),
              3: st([0.5, 1.25], [0.0])}
    steps = dga_stop_cpu.steps_of(states)
    assert np.array_equal(steps, [0.5, 2.0, 0.25, 0.0])
    assert dga_stop_cpu.stopping_iteration(steps, 0.5, 1) == 1
    assert dga_stop_cpu.stopping_iteration(steps, 0.5, 2) == 4          # iteration 2 is a check, but its step is 2.0
    assert dga_stop_cpu.stopping_iteration(steps, 0.0, 1) == 4          # an exact fixed point
    assert dga_stop_cpu.stopping_iteration(steps, 0.5, 1, after=1) == 3
    assert dga_stop_cpu.stop_state(steps, 0.1, 3, 4) == (4, False, 0.25)
    assert dga_stop_cpu.stop_state(steps, 0.5, 1, 4) == (1, True, 0.5)
    assert dga_stop_cpu.stop_state(steps, 0.1, 3, 2) == (2, False, np.inf)
    # a NaN that moves makes the step a NaN: never a stop; a kind that stands contributes 0 whatever it holds
    states[1] = st([0.5, 1.0], [np.nan])
    states[2] = st([0.5, 1.25], [np.nan])
    steps = dga_stop_cpu.steps_of(states)
    assert np.isnan(steps[1]) and steps[2] == 0.25
    assert dga_stop_cpu.stopping_iteration(steps[:2], 1e9, 2) is None
    only_eq = {-1: st([1.0], None), 0: st([3.0], None)}
    assert np.array_equal(dga_stop_cpu.steps_of(only_eq), [2.0])
    assert dga_stop_cpu.steps_of({-1: st([1.0], None)}).size == 0       # a dual-infeasible start has no iteration


def _lps():
    return [LP(*args) for args in fifteen()[:2]]


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    lps = _lps()
    golden = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    for tol in BAD_TOL:
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            dual_gradient_ascent_many_until(lps, tol)
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            solve_dga_many_until(golden, tol)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            dual_gradient_ascent_many_until(lps, TOL, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            solve_dga_many_until(golden, TOL, check_every=every)
    # the checks of the list itself stay those of dual_gradient_ascent_many
    with pytest.raises(ValueError, match="empty list"):
        dual_gradient_ascent_many_until([], TOL)
    with pytest.raises(ValueError, match="empty list"):
        solve_dga_many_until([], TOL)
    with pytest.raises(ValueError, match="LP 1 is not an LP object"):
        dual_gradient_ascent_many_until([lps[0], object()], TOL)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many_until(_lps(), 0.0, 1, nb_max_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_dga_many_until([lp_from_golden(load_golden("lp_potts8"), SparseLP)], TOL, nb_iter=3)


def test_names_and_signatures():
    for name in ("dual_gradient_ascent_many_until", "solve_dga_many_until", "DeviceDGAMany"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name), name
    assert str(inspect.signature(dual_gradient_ascent_many_until)) == (
        "(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None)")
    assert str(inspect.signature(solve_dga_many_until)) == "(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None)"
    assert pysparselp_amd.SparseLP.solve_dga_many_until is solve_dga_many_until
    assert str(inspect.signature(DeviceDGAMany.set_stop)) == "(self, tol, check_every=1)"
    assert str(inspect.signature(DeviceDGAMany.stop_state)) == "(self)"


def test_the_two_prototypes_are_declared_and_bound():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    assert "NO RESUME" in re.sub(r"\s+", " ", comments)   # the difference from slp_many_cp_set_stop is stated
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert "int slp_many_dual_set_stop(slp_many_dga *s, double tol, int64_t check_every);" in text
    assert "int slp_many_dual_stop_state(slp_many_dga *s, int64_t *iterations, int32_t *stopped, double *step);" in text
    lib = _lib.load()   # dlopen works without a GPU
    for name in ("slp_many_dual_set_stop", "slp_many_dual_stop_state"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.slp_many_dual_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_many_dual_stop_state.argtypes == [_lib.c_vp] * 4
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"C ABI ({len(_lib.EXPORTED_SYMBOLS)} entry points)" in readme


def test_the_draw_window_goes_on_without_a_stopped_reader(tmp_path):
    """Built and run as tests/test_dga_draws_host.py builds its program; nothing is loaded into Python."""
    exe = str(tmp_path / "dga_stop_window_main")
    cxx = os.environ.get("CXX", "g++")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", os.path.join(REPO, "pysparselp_amd", "csrc"), os.path.join(REPO, "tests", "host", "dga_stop_window_main.cpp"),
                            "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok:") and " 0 failures" in run.stdout
    assert run.stderr == ""


def test_the_stop_info_of_a_list_without_an_lp_left_out():
    """``dual_gradient_ascent_many_until`` solves every LP of its list: a frozen one is not stopped, and untested."""
    info = _many.new_stop_info(3, np.arange(3))
    assert not info["stopped"].any() and np.all(info["step"] == np.inf) and not info["iterations"].any()
    _many.spread_stop_state(info, np.arange(3), (np.array([20, 0, 130]), np.array([True, False, False]), np.array([1e-3, np.inf, 0.5])))
    assert np.array_equal(info["iterations"], [20, 0, 130]) and np.array_equal(info["stopped"], [True, False, False])
