"""Host side of the certificate the batched Chambolle-Pock solver can stop each instance on (``CPBatchState.set_stop_gap`` /
``gap_state``, ``chambolle_pock_ppd_batch_certified``, ``SparseLP.solve_batch_certified``): the names and the two prototypes of
include/slp_hip_ext.h are there and bound while include/slp_hip.h and its 215 entry points are untouched, the refusals come
before the library is touched, and the batches of tests/test_gpu_cp_batch_gap.py have what makes them a test -- every evaluated
check decidable, stops spread over the run, instances that do not stop, a wholly stopped tile beside a running one -- conditions
on the inputs, derived from the numpy restatement (tests/cp_gap_cpu.py) alone.  None of it needs a GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

import cp_gap_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden
from pysparselp_amd import _lib, chambolle_pock_ppd_batch_certified
from pysparselp_amd.ChambollePockPPD import CPBatchState
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401
from test_gpu_cp_batch import _instances, _of_instance

TOL_GAP = TOL_FEAS = 1e-2
EVERY = (1, 4, 10)
ITERATIONS = 200
LEFT_OUT = 0   # instances with an undecidable check: none
ALL_FOUR = ("c", "b", "bounds", "x0")

# name -> (fixture, B, what varies between the instances, seed)
BATCHES = {
    "potts8_1": ("potts8", 1, ("c",), 23),   # the fixture itself, alone
    "potts8_c": ("potts8", 5, ("c",), 23),
    "potts8_all": ("potts8", 5, ALL_FOUR, 74),
    "random1_c": ("random1", 5, ("c",), 24),
    "sc105_c": ("sc105", 5, ("c",), 23),
    "sc50a_all": ("sc50a", 5, ALL_FOUR, 74),
    "random0_cx0": ("random0", 8, ("c", "x0"), 11),
    "random2_cb": ("random2", 3, ("c", "b"), 11),
    "potts8_65": ("potts8", 65, ("c",), 11),
    "random1_65": ("random1", 65, ("c",), 11),
    "potts8_130": ("potts8", 130, ALL_FOUR, 11),
}
SMALL = ("potts8_1", "potts8_c", "potts8_all", "random1_c", "sc105_c", "sc50a_all", "random0_cx0", "random2_cb")
LARGE = ("potts8_65", "random1_65", "potts8_130")

# the stopping iterations per cadence (1, 4, 10), None: does not stop within ITERATIONS
STOPS = {
    "potts8_1": ([60], [60], [60]),
    "potts8_c": ([60, 68, 71, 50, 67], [60, 68, 72, 64, 68], [60, 80, 80, 50, 70]),
    "potts8_all": ([60, 112, 115, 96, 131], [60, 112, 116, 96, 132], [60, 120, 120, 100, 140]),
    "random1_c": ([174, None, 188, None, None], [176, None, 188, None, None], [180, None, 190, None, None]),
    "sc105_c": ([None] * 5,) * 3,
    "sc50a_all": ([None] * 5,) * 3,
}
# (instances that stop, first stop, last stop) per cadence
SPREAD = {
    "random0_cx0": ((8, 43, 54), (8, 44, 56), (8, 50, 60)),
    "random2_cb": ((1, 156, 156), (1, 156, 156), (1, 160, 160)),
    "potts8_65": ((65, 50, 100), (65, None, None), (65, None, None)),
    "random1_65": ((43, 133, 200), (43, 136, 200), (43, 140, 200)),
    "potts8_130": ((130, 60, 174), (130, 60, 176), (130, 60, 180)),
}
# instance 64, alone in tile 1, per cadence
LONE = {"potts8_65": (70, 72, 70), "random1_65": (159, 160, 160)}


@functools.lru_cache(maxsize=None)
def batch_args(name):
    """The arguments of ``chambolle_pock_ppd_batch`` for a batch of ``BATCHES`` (shared, never modified)."""
    case, batch, vary, seed = BATCHES[name]
    return _instances(load_golden("lp_" + case), batch, seed, vary)


@functools.lru_cache(maxsize=None)
def batch_certificates(name, nb_iter=ITERATIONS):
    """Per instance of the batch the restatement's certificates for ``t = 1 .. nb_iter`` (shared, read only)."""
    args = batch_args(name)
    out = []
    for k in range(BATCHES[name][1]):
        problem, x0 = _of_instance(args, k)
        out.append(cp_gap_cpu.certificates(problem, *cp_gap_cpu.iterates(problem, nb_iter, x0)))
    return tuple(out)


def batch_stops(name, every, total=ITERATIONS):
    return [cp_gap_cpu.stopping_iteration(cp_gap_cpu.Certificate(*(col[:total] for col in cert)), TOL_GAP, TOL_FEAS, every)
            for cert in batch_certificates(name)]


class _NoState(CPBatchState):
    """A state without a device: ``set_stop_gap`` must refuse before it looks for one."""

    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


def _lp():
    return lp_from_golden(load_golden("lp_potts8"), SparseLP)


def _call(name, *stop, **kw):
    a = batch_args(name)
    return chambolle_pock_ppd_batch_certified(a["c"], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"],
                                              *stop, x0=a["x0"], **kw)


def test_names_and_signatures():
    assert "chambolle_pock_ppd_batch_certified" in pysparselp_amd.__all__
    assert pysparselp_amd.chambolle_pock_ppd_batch_certified is chambolle_pock_ppd_batch_certified
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert all(hasattr(pysparselp_amd, name) for name in pysparselp_amd.__all__)
    assert str(inspect.signature(chambolle_pock_ppd_batch_certified)) == (
        "(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_gap, tol_feas, check_every=10, x0=None, alpha=1, theta=1, "
        "nb_max_iter=10000, callback_func=None, max_time=None, nb_iter_plot=10)")
    assert str(inspect.signature(SparseLP.solve_batch_certified)) == (
        "(self, costs, tol_gap, tol_feas, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10, "
        "ground_truth=None, ground_truth_indices=None)")
    assert str(inspect.signature(CPBatchState.set_stop_gap)) == "(self, tol_gap, tol_feas, check_every=1)"
    assert str(inspect.signature(CPBatchState.gap_state)) == "(self)"
    assert "fixed_cost" in SparseLP.solve_batch_certified.__doc__ and "remove_fixed_variables" in SparseLP.solve_batch_certified.__doc__
    for doc in (CPBatchState.set_stop_gap.__doc__, CPBatchState.gap_state.__doc__):
        assert "for the life of the state" in doc   # the one difference from the list solver


def test_the_two_prototypes_are_in_the_extension_header_and_bound():
    strip = lambda text: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))  # noqa: E731
    ext = strip(open(os.path.join(REPO, "include", "slp_hip_ext.h")).read())
    assert "int slp_cp_batch_set_stop_gap(slp_cp_batch *s, double tol_gap, double tol_feas, int64_t check_every);" in ext
    assert ("int slp_cp_batch_gap_state(slp_cp_batch *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, "
            "double *violation);") in ext
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_SYMBOLS) == ["slp_cp_batch_gap_state", "slp_cp_batch_set_stop_gap"]
    assert _lib.EXT_SYMBOLS == tuple(_lib._EXT_SIGNATURES)
    base = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    lib = _lib.load()   # dlopen works without a GPU
    for name in _lib.EXT_SYMBOLS:
        assert name not in base and name not in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.slp_cp_batch_set_stop_gap.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_cp_batch_gap_state.argtypes == [_lib.c_vp] * 6
    assert lib.slp_cp_batch_set_stop_gap.restype is _lib.c_int and lib.slp_cp_batch_gap_state.restype is _lib.c_int
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and "include/slp_hip_ext.h" in readme
    assert all(name in readme for name in _lib.EXT_SYMBOLS)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/slp_hip_ext.h") == makefile.count("../../include/slp_hip.h ") == 2


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    lp, st = _lp(), _NoState()
    costs = np.tile(lp.costsvector, (2, 1))
    for tol in BAD_TOL:
        for name, stop in (("tol_gap", (tol, 1e-2)), ("tol_feas", (1e-2, tol))):
            match = f"{name} must be a finite float >= 0"
            with pytest.raises(ValueError, match=match):
                _call("potts8_c", *stop)
            with pytest.raises(ValueError, match=match):
                lp.solve_batch_certified(costs, *stop)
            if not (name == "tol_gap" and tol is None):   # None is how the state's test is turned off
                with pytest.raises(ValueError, match=match):
                    st.set_stop_gap(*stop)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            _call("potts8_c", 1e-2, 1e-2, every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            lp.solve_batch_certified(costs, 1e-2, 1e-2, check_every=every)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            st.set_stop_gap(1e-2, 1e-2, every)
    # the checks of the batch itself stay those of chambolle_pock_ppd_batch / solve_batch
    a = batch_args("potts8_c")
    with pytest.raises(ValueError, match=r"expected \(B, n\)"):
        chambolle_pock_ppd_batch_certified(a["c"][0], a["a_eq"], a["beq"], a["a_ineq"], a["b_lower"], a["b_upper"], a["lb"], a["ub"],
                                           1e-2, 1e-2)
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_batch_certified(costs[:, :-1], 1e-2, 1e-2)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        _call("potts8_c", 0.0, 0.0, 1, nb_max_iter=3)
    lp = _lp()
    with pytest.raises(AssertionError, match="library was loaded"):
        lp.solve_batch_certified(np.tile(lp.costsvector, (2, 1)), 1e-2, 1e-2, nb_iter=3)


def test_a_batch_without_rows_is_stopped_after_no_iteration(no_library):  # noqa: F811
    rng = np.random.RandomState(5)
    n, batch = 4, 3
    c = rng.randn(batch, n)
    c[1, 2] = 0.0
    lb, ub = -rng.rand(n) - 1, rng.rand(batch, n) + 1
    called = []
    x, best, info = chambolle_pock_ppd_batch_certified(c, None, None, scipy.sparse.csr_matrix((0, n)), None, np.zeros(0), lb, ub, 1e-2, 1e-2,
                                                       callback_func=lambda *a: called.append(a))
    assert best == [None] * batch and not called
    assert sorted(info) == ["iterations", "lower_bound", "primal", "stopped", "violation"]
    assert info["iterations"].dtype == np.int64 and info["stopped"].dtype == bool
    assert all(info[name].dtype == np.float64 and info[name].shape == (batch,) for name in ("primal", "lower_bound", "violation"))
    assert np.array_equal(info["iterations"], [0] * batch) and np.array_equal(info["stopped"], [True] * batch)
    assert np.array_equal(x, np.where(c > 0, lb, np.where(c < 0, ub, 0.0)))
    for k in range(batch):
        assert info["primal"][k] == info["lower_bound"][k] == c[k].dot(x[k]) and info["violation"][k] == 0.0


def _condition(name, every):
    """Per instance its stopping iteration; asserts that every check the device evaluates is decidable."""
    certs = batch_certificates(name)
    stops = batch_stops(name, every)
    bands = []
    for cert, stop in zip(certs, stops):
        evaluated = cp_gap_cpu.checks(ITERATIONS if stop is None else stop, every)
        bands.append(min(cp_gap_cpu.bands_from_threshold(cert, t, TOL_GAP, TOL_FEAS) for t in evaluated))
    left_out = [k for k, cert in enumerate(certs) if not cp_gap_cpu.all_decidable(cert, TOL_GAP, TOL_FEAS, every, ITERATIONS)]
    print(name, "every", every, "stops", stops, "fewest bands from a threshold %.3g" % min(bands), "left out", left_out)
    assert len(left_out) <= LEFT_OUT and min(bands) > cp_gap_cpu.DECIDABLE_BANDS
    assert all(s is None or (s % every == 0 and 1 < s <= ITERATIONS) for s in stops)
    return stops


@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("name", SMALL)
def test_the_small_batches_are_decidable_and_stop_where_stated(name, every):
    """What makes the GPU cases a test at ``tol_gap = tol_feas = 1e-2`` over 200 iterations: every evaluated check of every
    instance is decidable and none is left out; the instances stop at different iterations, some batches mix stopped and
    running instances, and sc50a and sc105 do not stop."""
    stops = _condition(name, every)
    i = EVERY.index(every)
    if name in STOPS:
        assert stops == STOPS[name][i]
    else:
        reached = [s for s in stops if s is not None]
        assert (len(reached), min(reached), max(reached)) == SPREAD[name][i]
    if name == "potts8_c":   # the decision is not monotone in t: instance 3 stops at 50 but, checked every 4, only at 64
        assert batch_stops(name, 1)[3] == 50 and batch_stops(name, 4)[3] == 64 and batch_stops(name, 10)[3] == 50
    if name == "random2_cb":
        assert BATCHES[name][1] == 3   # Bt = 4: one padding instance


@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("name", LARGE)
def test_the_batches_of_more_than_one_tile_are_decidable_and_stop_where_stated(name, every):
    """65 instances are a full tile and a tile of one, 130 are 64 + 64 + 2.  potts8 at 65: instance 64 stops while tile 0 still
    runs -- a wholly stopped tile beside a running one; random1 at 65: tile 0 never wholly stops."""
    stops = _condition(name, every)
    i = EVERY.index(every)
    reached = [s for s in stops if s is not None]
    count, first, last = SPREAD[name][i]
    assert len(reached) == count
    if first is not None:
        assert (min(reached), max(reached)) == (first, last)
    if name in LONE:
        assert stops[64] == LONE[name][i]
    if name == "potts8_65":
        assert max(stops[:64]) == 100 and max(stops[:64]) > stops[64] + every
    if name == "random1_65":
        assert any(s is None for s in stops[:64])
    if name == "potts8_130":   # (between 60 and 180 a cadence of 10 leaves 13 places)
        assert len(set(reached)) >= 10
