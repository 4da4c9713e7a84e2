"""Host side of the per-instance stopping test of the batched dual gradient ascent (``dual_gradient_ascent_batch_until``,
``SparseLP.solve_dga_batch_until``, ``DeviceDGABatch.set_stop`` / ``stop_state``): the numpy restatement
(tests/dga_batch_stop_cpu.py) on hand-made curves, the refusals before the library is touched, the two prototypes in a header of
their own and bound, the new names and signatures.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import dga_batch_stop_cpu
import dga_stop_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from dga_batch_cases import batch_case
from dga_many_cases import LP
from pysparselp_amd import _batch, _lib, dual_gradient_ascent_batch, dual_gradient_ascent_batch_until
from pysparselp_amd.DualGradientAscent import DeviceDGABatch
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the CP form)

inf, nan = np.inf, np.nan
# iteration:         1    2    3     4     5      6     7     8     9    10
STEPS = np.array([[4.0, 2.0, 0.5, 0.25, 0.25, 0.125, 0.5, 0.0, 0.0, 0.0],      # 0: meets 0.25 at 4
                  [4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0],          # 1: never by step
                  [4.0, 2.0, 1.0, 0.25, 0.125, 0.125, 0.125, 0.125, 0.0, 0.0],  # 2: meets 0.25 at 4
                  [9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0],          # 3: never
                  [4.0, nan, nan, nan, nan, nan, nan, nan, nan, nan],          # 4: a NaN step
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])         # 5: never by step
BOUNDS = np.array([[-9.0, -5.0, -3.0, -2.0, -1.5, -1.25, -1.0, -1.0, -1.0, -1.0],   # 0: below its cut-off 0 throughout
                   [-9.0, -5.0, -3.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0, 3.0],           # 1: reaches 2.0 at 5
                   [-9.0, -5.0, -3.0, 7.0, 7.5, 8.0, 8.0, 8.0, 8.0, 8.0],           # 2: reaches 7.0 at 4, with its step
                   [-9.0, -8.0, -7.0, -6.0, -5.0, -4.0, -3.0, -2.0, -1.0, -0.5],    # 3: no cut-off
                   [-9.0, -5.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0],         # 4: a cut-off it would meet, but for the NaN bit
                   [nan, nan, nan, nan, nan, nan, nan, nan, nan, nan]])             # 5: a NaN bound
TARGETS = np.array([0.0, 2.0, 7.0, inf, 100.0, -50.0])


def same(got, iterations, stopped, step, bound, reason):
    assert got[0].dtype == np.int64 and got[1].dtype == bool and got[2].dtype == got[3].dtype == np.float64 and got[4].dtype == np.int32
    assert np.array_equal(got[0], iterations) and np.array_equal(got[1], stopped) and np.array_equal(got[4], reason), got
    assert np.array_equal(got[2], step, equal_nan=True) and np.array_equal(got[3], bound, equal_nan=True), got


def test_the_restatement_on_hand_made_curves():
    state = lambda rules, total, **kw: dga_batch_stop_cpu.stop_state(STEPS, BOUNDS, rules, total, **kw)  # noqa: E731
    # both tests at every iteration: step, bound, both at the same check, never, a NaN step, a NaN bound
    same(state([(0, 0.25, TARGETS, 1)], 10), [4, 5, 4, 10, 10, 10], [True, True, True, False, False, False],
         [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-2.0, 2.0, 7.0, -0.5, 4.0, nan], [1, 2, 3, 0, 0, 0])
    # the step alone: no bound is evaluated, so it stays -inf; instance 2 stops by its step only
    same(state([(0, 0.25, None, 1)], 10), [4, 10, 4, 10, 10, 10], [True, False, True, False, False, False],
         [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-inf] * 6, [1, 0, 1, 0, 0, 0])
    # the bound alone; a NaN bound meets nothing, not even -50
    same(state([(0, None, TARGETS, 1)], 10), [10, 5, 4, 10, 10, 10], [False, True, True, False, False, False],
         [0.0, 4.0, 0.25, 9.0, nan, 1.0], [-1.0, 2.0, 7.0, -0.5, 4.0, nan], [0, 2, 2, 0, 0, 0])
    # the cadence: checks at 3, 6, 9 only
    same(state([(0, 0.25, TARGETS, 3)], 10), [6, 6, 6, 10, 10, 10], [True, True, True, False, False, False],
         [0.125, 4.0, 0.125, 9.0, nan, 1.0], [-1.25, 3.0, 8.0, -1.0, 3.0, nan], [1, 2, 3, 0, 0, 0])
    # before the first check: +inf and -inf, for every instance
    same(state([(0, 0.25, TARGETS, 4)], 3), [3] * 6, [False] * 6, [inf] * 6, [-inf] * 6, [0] * 6)
    # armed when 7 iterations are complete, check_every = 5: the cadence counts over the life of the state, the first check is 10
    same(state([(7, 0.25, TARGETS, 5)], 9), [9] * 6, [False] * 6, [inf] * 6, [-inf] * 6, [0] * 6)
    same(state([(7, 0.25, TARGETS, 5)], 10), [10, 10, 10, 10, 10, 10], [True, True, True, False, False, False],
         [0.0, 4.0, 0.0, 9.0, nan, 1.0], [-1.0, 3.0, 8.0, -0.5, 4.0, nan], [1, 2, 3, 0, 0, 0])
    # the NaN bit: instance 4 would meet a cut-off of 1.0 at 7, its status carries the bit from 2 on
    t = TARGETS.copy()
    t[4] = 1.0
    assert state([(0, None, t, 1)], 10)[0][4] == 7
    got = state([(0, None, t, 1)], 10, nan_from=[None, None, None, None, 2, None])
    assert got[0][4] == 10 and not got[1][4] and got[3][4] == 4.0
    # a frozen instance has no iteration and is never stopped
    got = state([(0, 1e9, None, 1)], 10, frozen=[False, True, False, False, False, False])
    assert got[0].tolist() == [1, 0, 1, 1, 1, 1] and got[1].tolist() == [True, False, True, True, True, True]
    assert got[2][1] == inf and got[3][1] == -inf
    # sticky: a stopped instance stays stopped with its record when the rule is tightened, loosened or turned off
    same(state([(0, 0.25, None, 1), (5, 0.0, TARGETS, 1)], 10), [4, 6, 4, 10, 10, 10], [True, True, True, False, False, False],
         [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-inf, 3.0, -inf, -0.5, 4.0, nan], [1, 2, 1, 0, 0, 0])
    same(state([(0, 0.25, None, 1), (5, None, None, 1)], 10), [4, 10, 4, 10, 10, 10], [True, False, True, False, False, False],
         [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-inf] * 6, [1, 0, 1, 0, 0, 0])
    # three rules -- armed in mid-life, armed again with other cut-offs and another cadence, turned off: rule 1 (after 2, checks 3, 4)
    # stops 0 and 2 by their step at 4 and records 1.0 for instance 1; rule 2 (after 4, cadence 2: the check 6) stops 1 by its new
    # cut-off 3.0 and 5 by the looser tolerance 1.0; rule 3 (after 7) evaluates nothing, every record stays
    t2 = np.array([inf, 3.0, inf, inf, inf, inf])
    rules = [(2, 0.25, TARGETS, 1), (4, 1.0, t2, 2), (7, None, None, 1)]
    same(state(rules, 2), [2] * 6, [False] * 6, [inf] * 6, [-inf] * 6, [0] * 6)
    same(state(rules, 4), [4, 4, 4, 4, 4, 4], [True, False, True, False, False, False],
         [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-2.0, 1.0, 7.0, -6.0, -2.0, nan], [1, 0, 3, 0, 0, 0])
    for total in (7, 10):
        same(state(rules, total), [4, 6, 4, total, total, 6], [True, True, True, False, False, True],
             [0.25, 4.0, 0.25, 9.0, nan, 1.0], [-2.0, 3.0, 7.0, -4.0, 0.0, nan], [1, 2, 3, 0, 0, 1])
    # ... with a frozen instance in the middle: no iteration, no record, under every rule
    got = state(rules, 10, frozen=[False, False, True, False, False, False])
    assert (got[0][2], got[1][2], got[2][2], got[3][2], got[4][2]) == (0, False, inf, -inf, 0) and got[0][[0, 1, 5]].tolist() == [4, 6, 6]
    # a scalar cut-off is every instance's
    assert state([(0, None, 2.5, 1)], 10)[0].tolist() == [10, 6, 4, 10, 9, 10]


def test_the_restatement_is_built_on_the_list_solvers():
    assert dga_batch_stop_cpu.steps_of is dga_stop_cpu.steps_of and dga_batch_stop_cpu.stopping_iteration is dga_stop_cpu.stopping_iteration
    # with a step test alone an instance is an LP of the list
    for k in range(6):
        for tol, every, total in ((0.25, 1, 10), (0.125, 3, 10), (0.25, 4, 3)):
            got = dga_batch_stop_cpu.stop_state(STEPS[k:k + 1], BOUNDS[k:k + 1], [(0, tol, None, every)], total)
            want = dga_stop_cpu.stop_state(STEPS[k], tol, every, total)
            assert (got[0][0], got[1][0]) == want[:2] and np.array_equal(got[2][0], want[2], equal_nan=True)

    def st(y_eq, y_ineq):
        return (None, np.array(y_eq, dtype=np.float64), np.array(y_ineq, dtype=np.float64), 0)

    states = {-1: st([0.0, 1.0], [2.0]), 0: st([0.5, 1.0], [2.0]), 1: st([0.5, 1.0], [0.0])}
    steps, bounds = dga_batch_stop_cpu.curves_of(states, lambda y_eq, y_ineq: float(y_eq.sum() - y_ineq.sum()))
    assert np.array_equal(steps, [0.5, 2.0]) and np.array_equal(bounds, [-0.5, 1.5])


class _NoState(DeviceDGABatch):
    """A state without a device: ``set_stop`` must refuse before it looks for one."""

    batch = 6

    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


def _lp():
    args, costs = batch_case("sc50a")
    return LP(*args), costs


BAD_TARGETS = ([1.0, 2.0], np.zeros((6, 1)), np.zeros((2, 3)), [0.0, 1.0, nan, 3.0, 4.0, 5.0], [0.0, 1.0, -inf, 3.0, 4.0, 5.0], nan, -inf,
               "3", [True] * 6, 1j)


def test_a_bad_rule_is_refused_before_the_library(no_library):  # noqa: F811
    lp, costs = _lp()
    golden = lp_from_golden(load_golden("lp_sc50a"), SparseLP)
    st = _NoState()
    with pytest.raises(ValueError, match="needs tol, targets or both"):
        dual_gradient_ascent_batch_until(lp, costs)
    with pytest.raises(ValueError, match="needs tol, targets or both"):
        golden.solve_dga_batch_until(costs)
    for tol in BAD_TOL:
        if tol is None:   # None is "no step test": refused only when there is no bound test either
            continue
        for targets in (None, 1.0):
            with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
                dual_gradient_ascent_batch_until(lp, costs, tol, targets)
            with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
                golden.solve_dga_batch_until(costs, tol, targets)
            with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
                st.set_stop(tol, targets)
    for every in BAD_EVERY:
        for rule in ((1e-2, None), (None, 1.0), (1e-2, np.zeros(6))):
            with pytest.raises(ValueError, match="check_every must be an int >= 1"):
                dual_gradient_ascent_batch_until(lp, costs, *rule, every)
            with pytest.raises(ValueError, match="check_every must be an int >= 1"):
                golden.solve_dga_batch_until(costs, *rule, check_every=every)
            with pytest.raises(ValueError, match="check_every must be an int >= 1"):
                st.set_stop(*rule, every)
    for targets in BAD_TARGETS:
        for tol in (None, 1e-2):
            with pytest.raises(ValueError, match="^targets "):
                dual_gradient_ascent_batch_until(lp, costs, tol, targets)
            with pytest.raises(ValueError, match="^targets "):
                golden.solve_dga_batch_until(costs, tol, targets)
            with pytest.raises(ValueError, match="^targets "):
                st.set_stop(tol, targets)
        with pytest.raises(ValueError, match="^targets "):
            _batch.check_targets(targets, 6)
    # what is accepted: a scalar for all, one per instance, +inf for an instance without a cut-off
    assert _batch.check_targets(None, 6) is None
    assert np.array_equal(_batch.check_targets(3, 6), [3.0] * 6) and np.array_equal(_batch.check_targets(np.float32(0.5), 2), [0.5, 0.5])
    got = _batch.check_targets([0, inf, -1.5], 3)
    assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, [0.0, inf, -1.5])
    # the checks of the batch itself stay those of dual_gradient_ascent_batch / solve_dga_batch
    with pytest.raises(ValueError, match="costs has shape"):
        dual_gradient_ascent_batch_until(lp, costs[:, :-1], 1e-2)
    with pytest.raises(ValueError, match="costs has shape"):
        golden.solve_dga_batch_until(costs[0], 1e-2)
    two_sided = LP(*batch_case("sc50a")[0])
    two_sided.b_lower = np.zeros(two_sided.b_upper.size)
    with pytest.raises(ValueError, match="one-sided"):
        dual_gradient_ascent_batch_until(two_sided, costs, 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    lp, costs = _lp()
    for rule in ((0.0, None, 1), (None, 0, 3), (np.float32(0.5), [inf] * 6, np.int64(2))):
        with pytest.raises(AssertionError, match="library was loaded"):
            dual_gradient_ascent_batch_until(lp, costs, *rule, nb_max_iter=3)
    golden = lp_from_golden(load_golden("lp_sc50a"), SparseLP)
    with pytest.raises(AssertionError, match="library was loaded"):
        golden.solve_dga_batch_until(costs, targets=np.zeros(6), nb_iter=3)


def test_names_and_signatures():
    assert "dual_gradient_ascent_batch_until" in pysparselp_amd.__all__ and "DeviceDGABatch" in pysparselp_amd.__all__
    assert pysparselp_amd.dual_gradient_ascent_batch_until is pysparselp_amd.DualGradientAscent.dual_gradient_ascent_batch_until
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert all(hasattr(pysparselp_amd, name) for name in pysparselp_amd.__all__)
    assert "dual_gradient_ascent_batch_until" in pysparselp_amd.__doc__ and "solve_dga_batch_until" in pysparselp_amd.__doc__
    assert str(inspect.signature(dual_gradient_ascent_batch_until)) == (
        "(lp, costs, tol=None, targets=None, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, "
        "lower_bounds=None, upper_bounds=None, path=None)")
    assert str(inspect.signature(SparseLP.solve_dga_batch_until)) == (
        "(self, costs, tol=None, targets=None, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10, "
        "ground_truth=None, ground_truth_indices=None, lower_bounds=None, upper_bounds=None)")
    assert str(inspect.signature(DeviceDGABatch.set_stop)) == "(self, tol, targets=None, check_every=1)"
    assert str(inspect.signature(DeviceDGABatch.stop_state)) == "(self)"
    for doc in (DeviceDGABatch.set_stop.__doc__, dual_gradient_ascent_batch_until.__doc__):
        assert "cannot be resumed" in " ".join(doc.split()) or "takes no part in later launches" in " ".join(doc.split())
    # dual_gradient_ascent_batch and solve_dga_batch keep their signatures
    assert str(inspect.signature(dual_gradient_ascent_batch)) == (
        "(lp, costs, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, lower_bounds=None, upper_bounds=None, "
        "path=None)")
    assert str(inspect.signature(SparseLP.solve_dga_batch)) == (
        "(self, costs, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10, ground_truth=None, ground_truth_indices=None, "
        "lower_bounds=None, upper_bounds=None)")


def test_the_two_prototypes_are_in_a_header_of_their_own_and_bound():
    strip = lambda text: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))  # noqa: E731
    include = os.path.join(REPO, "include")
    assert '#include "slp_hip_ext_dga_batch.h"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = strip(open(os.path.join(include, "slp_hip_ext_dga_batch.h")).read())
    assert "int slp_batch_dga_set_stop(slp_batch_dga *s, double tol, const double *targets, int64_t check_every);" in ext
    assert "int slp_batch_dga_stop_state(slp_batch_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound);" in ext
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    new = list(_lib.EXT_DGA_BATCH_SYMBOLS)
    assert declared == sorted(new) == ["slp_batch_dga_set_stop", "slp_batch_dga_stop_state"]
    assert _lib.EXT_DGA_BATCH_SYMBOLS == tuple(_lib._EXT_DGA_BATCH_SIGNATURES)
    # ... and nowhere else: not in slp_hip.h, whose 215 entry points stay, nor in the text of the other extension headers
    for other in ("slp_hip.h", "slp_hip_ext.h", "slp_hip_ext_admm_batch.h"):
        text = strip(open(os.path.join(include, other)).read())
        assert not any(name in text for name in new), other
    base = open(os.path.join(include, "slp_hip.h")).read()
    lib = _lib.load()   # dlopen works without a GPU
    for name in new:
        assert name not in base and name not in _lib.EXPORTED_SYMBOLS and name not in _lib.EXT_SYMBOLS, name
        assert name not in _lib.EXT_ADMM_BATCH_SYMBOLS and hasattr(lib, name), name
    assert lib.slp_batch_dga_set_stop.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_vp, _lib.c_i64]
    assert lib.slp_batch_dga_stop_state.argtypes == [_lib.c_vp] * 5
    assert lib.slp_batch_dga_set_stop.restype is _lib.c_int and lib.slp_batch_dga_stop_state.restype is _lib.c_int
    assert len(_lib.EXPORTED_SYMBOLS) == 215   # include/slp_hip.h stays as it is
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and "slp_hip_ext_dga_batch.h" in readme
    assert all(name in readme for name in new) and "dual_gradient_ascent_batch_until" in readme
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/slp_hip_ext_dga_batch.h") == 2   # both dependency lists
