"""Host side of the certificate as the stopping test of the single Chambolle-Pock solver (``slp_cp_set_stop_gap``,
include/slp_hip_ext_cp_gap.h; ``CPState`` / ``DeviceCP`` ``.certificate`` / ``.set_stop_gap`` / ``.gap_state``,
``chambolle_pock_ppd_certified``, ``SparseLP.solve_certified``): the refusals come before the library is touched, an LP without
rows returns its box vertex, the three prototypes sit in a header of their own and are bound in a table of their own, and the
inputs of tests/test_gpu_cp_gap_single.py are pinned on the numpy restatement (tests/cp_gap_cpu.py).  None of it needs a GPU."""
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
from pysparselp_amd import _lib
from pysparselp_amd.ChambollePockPPD import CPState, chambolle_pock_ppd, chambolle_pock_ppd_certified
from pysparselp_amd.scale import DeviceCP
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the list form)
from test_oracle_golden import _reduced

ITERATIONS = 400
# fixture -> ((tol_gap, tol_feas), stopping iteration at check_every = 1, at check_every = 10); None: no stop in ITERATIONS
TABLE = (
    ("lp_potts8", (1e-2, 1e-2), 60, 60),
    ("lp_potts8", (1e-3, 1e-3), 96, 100),
    ("lp_random0", (1e-2, 1e-2), 47, 50),
    ("lp_random1", (1e-2, 1e-2), 174, 180),
    ("lp_random2", (1e-2, 1e-2), 156, 160),
    ("lp_sc50a", (1e-2, 1e-2), None, None),
)
NEW = ["slp_cp_certificate", "slp_cp_gap_state", "slp_cp_set_stop_gap"]
HEADER = "slp_hip_ext_cp_gap.h"
PROTOTYPES = (
    "int slp_cp_certificate(slp_cp *s, double out[3]);",
    "int slp_cp_set_stop_gap(slp_cp *s, double tol_gap, double tol_feas, int64_t check_every);",
    "int slp_cp_gap_state(slp_cp *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);",
)


@functools.lru_cache(maxsize=None)
def problem_of(name):
    return _reduced(load_golden(name))


@functools.lru_cache(maxsize=None)
def certificates_of(name, nb_iter=ITERATIONS):
    """``(xs, ys, certificates)`` of the restatement for ``t = 1 .. nb_iter`` (shared, read only)."""
    xs, ys = cp_gap_cpu.iterates(problem_of(name), nb_iter)
    return xs, ys, cp_gap_cpu.certificates(problem_of(name), xs, ys)


class _NoState(CPState):
    """A state without a device: ``set_stop_gap`` must refuse before it looks for one."""

    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


class _NoDeviceState(DeviceCP):
    def __init__(self):
        pass

    def close(self):
        pass

    __del__ = close


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    p = problem_of("lp_random1")
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    states = (_NoState(), _NoDeviceState())
    for tol in BAD_TOL:
        for name, args in (("tol_gap", (tol, 1e-2)), ("tol_feas", (1e-2, tol))):
            match = f"{name} must be a finite float >= 0"
            for setup in ("host", "device"):
                with pytest.raises(ValueError, match=match):
                    chambolle_pock_ppd_certified(*p, *args, setup=setup)
                with pytest.raises(ValueError, match=match):
                    lp.solve_certified(*args, setup=setup)
            if not (name == "tol_gap" and tol is None):   # None is how the state's test is turned off
                for st in states:
                    with pytest.raises(ValueError, match=match):
                        st.set_stop_gap(*args)
    for every in BAD_EVERY:
        match = "check_every must be an int >= 1"
        with pytest.raises(ValueError, match=match):
            chambolle_pock_ppd_certified(*p, 1e-2, 1e-2, every)
        with pytest.raises(ValueError, match=match):
            lp.solve_certified(1e-2, 1e-2, check_every=every)
        for st in states:
            with pytest.raises(ValueError, match=match):
                st.set_stop_gap(1e-2, 1e-2, every)
    assert not hasattr(lp, "stop_info")


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        chambolle_pock_ppd_certified(*problem_of("lp_random1"), 0.0, 0.0, 1, nb_max_iter=3, setup="host")
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_from_golden(load_golden("lp_potts8"), SparseLP).solve_certified(1e-2, 1e-2, nb_iter=3, setup="host")


def test_an_lp_without_rows_returns_its_box_vertex_stopped(no_library):  # noqa: F811
    rng = np.random.RandomState(5)
    for n, rows in ((4, scipy.sparse.csr_matrix((0, 4))), (1, None)):
        c = rng.randn(n)
        c[0] = 0.0 if n > 1 else c[0]
        lb, ub = -rng.rand(n) - 1, rng.rand(n) + 1
        x, best, info = chambolle_pock_ppd_certified(c, None, None, rows, None, np.zeros(0), lb, ub, 1e-2, 1e-2)
        assert best is None and np.array_equal(x, np.where(c > 0, lb, np.where(c < 0, ub, 0.0)))
        assert info == dict(iterations=0, stopped=True, primal=c.dot(x), lower_bound=c.dot(x), violation=0.0)
        assert np.array_equal(x, chambolle_pock_ppd(c, None, None, rows, None, np.zeros(0), lb, ub))   # as before: the vertex alone


def test_names_and_signatures():
    assert "chambolle_pock_ppd_certified" in pysparselp_amd.__all__ and hasattr(pysparselp_amd, "chambolle_pock_ppd_certified")
    assert "chambolle_pock_ppd_certified" in pysparselp_amd.__doc__ and len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert str(inspect.signature(chambolle_pock_ppd_certified)) == (
        "(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_gap, tol_feas, check_every=10, x0=None, alpha=1, theta=1, "
        "nb_max_iter=10000, callback_func=None, max_time=None, nb_iter_plot=10, order=0, setup='auto')")
    assert str(inspect.signature(SparseLP.solve_certified)) == (
        "(self, tol_gap, tol_feas, check_every=10, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10, "
        "ground_truth=None, ground_truth_indices=None, order=0, setup='auto')")
    for cls in (CPState, DeviceCP):
        assert str(inspect.signature(cls.certificate)) == "(self)"
        assert str(inspect.signature(cls.set_stop_gap)) == "(self, tol_gap, tol_feas, check_every=1)"
        assert str(inspect.signature(cls.gap_state)) == "(self)"
    assert str(inspect.signature(DeviceCP.y)) == "(self)"
    assert "fixed_cost" in SparseLP.solve_certified.__doc__ and "remove_fixed_variables" in SparseLP.solve_certified.__doc__
    # solve and chambolle_pock_ppd keep their signatures
    assert list(inspect.signature(SparseLP.solve).parameters)[:5] == ["self", "method", "get_timing", "x0", "nb_iter"]
    assert list(inspect.signature(chambolle_pock_ppd).parameters)[-3:] == ["nb_iter_plot", "order", "setup"]


def _strip(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_three_prototypes_are_in_a_header_of_their_own_and_bound():
    include = os.path.join(REPO, "include")
    assert f'#include "{HEADER}"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = _strip(open(os.path.join(include, HEADER)).read())
    for prototype in PROTOTYPES:
        assert prototype in ext, prototype
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_CP_GAP_SYMBOLS) == NEW
    assert _lib.EXT_CP_GAP_SYMBOLS == tuple(_lib._EXT_CP_GAP_SIGNATURES)
    for other in sorted(os.listdir(include)):   # ... and in no other header
        if other != HEADER:
            text = _strip(open(os.path.join(include, other)).read())
            assert not any(re.search(r"\b" + name + r"\b", text) for name in NEW), other
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    others = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.EXT_ADMM_BATCH_SYMBOLS, _lib.EXT_DGA_BATCH_SYMBOLS, _lib.EXT_DGA_MANY_SYMBOLS,
              _lib.EXT_DGA_MANY_LIVE_SYMBOLS, _lib.EXT_MANY_LIVE_SYMBOLS, _lib.EXT_TALL_SYMBOLS, _lib.EXT_BATCH_RHS_SYMBOLS)
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert all(name not in table for table in others), name
        assert getattr(lib, name).restype is _lib.c_int
    assert lib.slp_cp_certificate.argtypes == [_lib.c_vp, _lib.c_vp]
    assert lib.slp_cp_set_stop_gap.argtypes == [_lib.c_vp, _lib.c_dbl, _lib.c_dbl, _lib.c_i64]
    assert lib.slp_cp_gap_state.argtypes == [_lib.c_vp] * 6
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and HEADER in readme and all(name in readme for name in NEW)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/" + HEADER) == 2   # both dependency lists


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    out = np.zeros(3)
    assert lib.slp_cp_certificate(None, _lib.ptr(out)) != 0
    assert lib.slp_cp_set_stop_gap(None, 1e-2, 1e-2, 1) != 0 and b"NULL handle" in lib.slp_last_error()
    assert lib.slp_cp_gap_state(None, None, None, None, None, None) != 0 and b"NULL handle" in lib.slp_last_error()


@pytest.mark.parametrize("name, tol, stop1, stop10", TABLE)
def test_the_inputs_of_the_gpu_cases_on_the_restatement(name, tol, stop1, stop10):
    """Where every fixture stops, and that every check up to there is decidable: the GPU test compares stopping iterations and
    decisions exactly."""
    _, _, cert = certificates_of(name)
    assert len(cert.primal) == ITERATIONS
    for every, want in ((1, stop1), (10, stop10)):
        assert cp_gap_cpu.stopping_iteration(cert, *tol, every) == want, every
        assert cp_gap_cpu.all_decidable(cert, *tol, every, ITERATIONS), every
    for every in (1, 4, 10):   # the cadences of the GPU test's cuts
        assert cp_gap_cpu.all_decidable(cert, *tol, every, ITERATIONS)
        if name == "lp_random1":   # ... which also run 200 iterations of it with tolerances of 0: never met
            assert cp_gap_cpu.all_decidable(cert, 0.0, 0.0, every, 200)
            assert cp_gap_cpu.gap_state(cert, 0.0, 0.0, every, 200)[:2] == (200, False)
