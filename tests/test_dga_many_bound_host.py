"""Host side of the bound cut-off of dual gradient ascent on a list (``slp_many_dual_set_cutoff`` / ``slp_many_dual_cutoff_state``,
``DeviceDGAMany.set_cutoff`` / ``stop_state_full``, ``dual_gradient_ascent_many_cutoff``, ``solve_dga_many_cutoff``): the two
prototypes are in a header of their own and bound in a table of their own while slp_hip.h, its 215 entry points and the existing
Python signatures stay; bad arguments are refused before the library is touched; and the cases tests/test_gpu_dga_many_bound.py
relies on (tests/dga_many_bound_cases.py) have, by the numpy restatement alone, every way of stopping at every cadence.  None of
it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import dga_batch_stop_cpu
import dga_many_bound_cases as cases
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from dga_many_cases import LP
from pysparselp_amd import _lib, dual_gradient_ascent_many_cutoff, dual_gradient_ascent_many_until, solve_dga_many_cutoff, solve_dga_many_until
from pysparselp_amd.DualGradientAscent import DeviceDGAMany
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401
from test_dga_many_stop_host import ITERATIONS, fifteen, fifteen_states

NEW = ["slp_many_dual_cutoff_state", "slp_many_dual_set_cutoff"]


# ------------------------------------------------------------------ header, bindings, signatures
def test_the_two_prototypes_are_in_a_header_of_their_own_and_bound():
    strip = lambda text: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))  # noqa: E731
    include = os.path.join(REPO, "include")
    assert '#include "slp_hip_ext_dga_many.h"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = strip(open(os.path.join(include, "slp_hip_ext_dga_many.h")).read())
    assert "int slp_many_dual_set_cutoff(slp_many_dga *s, double tol, const double *targets, int64_t check_every);" in ext
    assert "int slp_many_dual_cutoff_state(slp_many_dga *s, int64_t *iterations, int32_t *reason, double *step, double *bound);" in ext
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_DGA_MANY_SYMBOLS) == NEW
    assert _lib.EXT_DGA_MANY_SYMBOLS == tuple(_lib._EXT_DGA_MANY_SIGNATURES)
    # ... and in no other header; slp_hip.h keeps its 215 entry points and the two existing names
    for other in sorted(os.listdir(include)):
        if other != "slp_hip_ext_dga_many.h":
            text = strip(open(os.path.join(include, other)).read())
            assert not any(name in text for name in NEW), other
    base = strip(open(os.path.join(include, "slp_hip.h")).read())
    assert "int slp_many_dual_set_stop(slp_many_dga *s, double tol, int64_t check_every);" in base
    assert "int slp_many_dual_stop_state(slp_many_dga *s, int64_t *iterations, int32_t *stopped, double *step);" in base
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        for table in (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.EXT_ADMM_BATCH_SYMBOLS, _lib.EXT_DGA_BATCH_SYMBOLS, _lib.EXT_TALL_SYMBOLS):
            assert name not in table, name
    assert lib.slp_many_dual_set_cutoff.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_vp, _lib.c_i64]
    assert lib.slp_many_dual_cutoff_state.argtypes == [_lib.c_vp] * 5
    assert lib.slp_many_dual_set_cutoff.restype is _lib.c_int and lib.slp_many_dual_cutoff_state.restype is _lib.c_int
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and "slp_hip_ext_dga_many.h" in readme
    assert all(name in readme for name in NEW) and "dual_gradient_ascent_many_cutoff" in readme
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/slp_hip_ext_dga_many.h") == 2   # both dependency lists


def test_names_and_signatures():
    for name in ("dual_gradient_ascent_many_cutoff", "solve_dga_many_cutoff"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name) and name in pysparselp_amd.__doc__, name
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert str(inspect.signature(dual_gradient_ascent_many_cutoff)) == (
        "(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None, targets=None)")
    assert str(inspect.signature(solve_dga_many_cutoff)) == (
        "(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None, targets=None)")
    assert pysparselp_amd.SparseLP.solve_dga_many_cutoff is solve_dga_many_cutoff
    assert str(inspect.signature(DeviceDGAMany.set_cutoff)) == "(self, tol, check_every=1, targets=None)"
    assert str(inspect.signature(DeviceDGAMany.stop_state_full)) == "(self)"
    # the forms without cut-offs keep their signatures
    assert str(inspect.signature(dual_gradient_ascent_many_until)) == (
        "(lps, tol, check_every=10, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None)")
    assert str(inspect.signature(solve_dga_many_until)) == "(lps, tol, check_every=10, get_timing=True, nb_iter=10000, max_time=None)"
    assert str(inspect.signature(DeviceDGAMany.set_stop)) == "(self, tol, check_every=1)"
    assert str(inspect.signature(DeviceDGAMany.stop_state)) == "(self)"


# ------------------------------------------------------------------ refusals before the library
def test_bad_arguments_are_refused_before_the_library(no_library):  # noqa: F811
    lps = [LP(*args) for args in fifteen()[:2]]
    golden = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    with pytest.raises(ValueError, match="both are None"):
        dual_gradient_ascent_many_cutoff(lps, None)
    for bad in (np.nan, -np.inf, [0.0, np.nan], [0.0, -np.inf]):
        with pytest.raises(ValueError, match="NaN or -inf"):
            dual_gradient_ascent_many_cutoff(lps, None, targets=bad)
    for bad in ([0.0, 1.0, 2.0], np.zeros((2, 1)), "1.0", [True, False]):
        with pytest.raises(ValueError, match="targets"):
            dual_gradient_ascent_many_cutoff(lps, 1e-3, targets=bad)
    with pytest.raises(ValueError, match="targets has shape"):
        solve_dga_many_cutoff(golden, None, targets=[1.0, 2.0])
    for tol in BAD_TOL:
        if tol is None:
            continue   # None is "no step test" once cut-offs are given
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            dual_gradient_ascent_many_cutoff(lps, tol, targets=0.0)
        with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
            solve_dga_many_cutoff(golden, tol, targets=0.0)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            dual_gradient_ascent_many_cutoff(lps, None, every, targets=0.0)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            solve_dga_many_cutoff(golden, 1e-3, check_every=every, targets=0.0)
    # without cut-offs the refusals are those of the forms they fall back on
    with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
        dual_gradient_ascent_many_cutoff(lps, -1.0)
    with pytest.raises(ValueError, match="both are None"):
        solve_dga_many_cutoff(golden, None)
    with pytest.raises(ValueError, match="empty list"):
        dual_gradient_ascent_many_cutoff([], None, targets=0.0)
    with pytest.raises(ValueError, match="empty list"):
        solve_dga_many_cutoff([], None, targets=0.0)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    lps = [LP(*args) for args in fifteen()[:2]]
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many_cutoff(lps, None, 1, nb_max_iter=3, targets=[0.0, np.inf])
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_dga_many_cutoff([lp_from_golden(load_golden("lp_potts8"), SparseLP)], 1e-3, nb_iter=3, targets=5)


# ------------------------------------------------------------------ the cases of the GPU test, by the restatement alone
def test_the_device_order_of_sums_stays_within_the_rounding_of_the_energy():
    for args, states in zip(fifteen(), fifteen_states()):
        for t in range(1, ITERATIONS + 1):
            assert cases.energies_agree(args, states[t - 1][1], states[t - 1][2]), t


@pytest.mark.parametrize("every", cases.EVERY)
def test_the_chosen_cut_offs_give_every_way_of_stopping(every):
    curves, targets = cases.fifteen_curves(), cases.targets()
    iterations, stopped, step, bound, reason = cases.expected([(0, cases.TOL, targets, every)])
    print("iterations", iterations, "reason", reason)
    assert (reason == 2).sum() >= 3 and (reason == 1).sum() >= 3 and (reason == 3).sum() >= 1
    assert (~stopped).sum() >= 2 and np.all(iterations[~stopped] == ITERATIONS)
    assert np.array_equal(stopped, reason != 0)
    # one LP has the tolerance's own check and its own bound at the same check
    k = cases.BOTH
    assert reason[k] == 3 and iterations[k] == cases.EQUAL[k] and bound[k] == targets[k] and step[k] <= cases.TOL
    # >= decides by equality ...
    equal = [j for j, check in cases.EQUAL.items() if iterations[j] == check and bound[j] == targets[j] and reason[j] & 2]
    assert len(equal) >= 2, equal
    # ... and a cut-off one ulp above the bound of a check is reached there and not met: the LP goes past that check
    for j, check in cases.ABOVE.items():
        b = curves[j][1][check - 1]
        assert targets[j] == np.nextafter(b, np.inf) > b and iterations[j] > check, j
    assert len(cases.ABOVE) >= 2
    # a finite cut-off out of reach, and none at all: the bound is recorded at the last check all the same
    last = ITERATIONS - ITERATIONS % every
    for j in cases.NEVER:
        assert not stopped[j] and bound[j] == curves[j][1][last - 1], j
    free = [j for j in range(15) if targets[j] == np.inf]
    assert len(free) >= 3 and all(np.isfinite(bound[j]) and not reason[j] & 2 for j in free)
    assert any(not stopped[j] for j in free)
    # without the tolerance the step is recorded and not tested
    without = cases.expected([(0, None, targets, every)])
    assert not (without[4] & 1).any() and np.all(np.isfinite(without[2]))
    assert all(without[0][j] == ITERATIONS for j in free)


def test_the_restatement_follows_a_change_of_rule():
    rules = cases.schedule()
    ends = [cases.expected(list(rules[:i + 1]), total=(rules[i + 1][0] if i + 1 < len(rules) else cases.SCHEDULE_TOTAL)) for i in range(len(rules))]
    first, second, third, last = ends
    print("iterations", [e[0].tolist() for e in ends])
    # armed at 7 with cadence 10: the checks are 10 and 20; LPs 7 and 10 stop at 20 on their bounds
    assert first[0][7] == first[0][10] == 20 and first[4][7] == first[4][10] == 2 and first[0].max() == 26
    # from 26 on the checks are 28, 32, 36: the new cut-offs stop LPs 0, 6 and 2 there, LP 2 at the rule's last check
    assert (second[0][0], second[0][6], second[0][2]) == (28, 32, 36) and second[4][[0, 6, 2]].tolist() == [2, 2, 2]
    moving = ~second[1]
    assert moving.sum() >= 4
    # from 36 on the tolerance alone: the bounds recorded stay those of check 36, LP 3 stops on its step at 40
    assert third[0][3] == 40 and third[4][3] == 1
    assert np.array_equal(third[3][moving], second[3][moving]) and np.all(np.isfinite(third[3][moving]))
    # off at 50: the records stay, the moving LPs count on
    for a, b in zip(third[1:], last[1:]):
        assert np.array_equal(a, b)
    still = ~third[1]
    assert np.all(last[0][still] == cases.SCHEDULE_TOTAL) and np.array_equal(last[0][~still], third[0][~still])
    # a stopped LP stays stopped under every later rule
    for before, after in zip(ends, ends[1:]):
        assert np.array_equal(after[0][before[1]], before[0][before[1]]) and np.array_equal(after[4][before[1]], before[4][before[1]])


def test_the_restatement_on_hand_made_curves():
    steps = [np.array([1.0, 0.5, 0.25, 0.0]), np.array([1.0, 1.0, np.nan, 1.0])]
    bounds = [np.array([-4.0, -2.0, -1.0, -1.0]), np.array([0.0, 1.0, 2.0, np.nan])]
    got = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, None, np.array([-1.0, 5.0]), 1)], 4)
    assert got[0].tolist() == [3, 4] and got[4].tolist() == [2, 0] and got[3][0] == -1.0 and np.isnan(got[3][1]) and got[2][1] == 1.0
    got = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, 0.25, np.array([-1.0, np.inf]), 1)], 4)
    assert got[0].tolist() == [3, 4] and got[4].tolist() == [3, 0]
    got = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, 0.25, np.array([-1.0, 2.0]), 2)], 4, nan_from=[None, 3])
    assert got[0].tolist() == [4, 4] and got[4].tolist() == [3, 0]   # a NaN bit from iteration 3 on meets nothing
    got = dga_batch_stop_cpu.stop_state(steps, bounds, [(0, 0.25, np.array([-1.0, 2.0]), 2)], 4, frozen=[True, False])
    assert got[0].tolist() == [0, 4] and got[3][0] == -np.inf and got[2][0] == np.inf
