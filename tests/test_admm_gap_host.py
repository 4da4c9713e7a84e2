"""Host side of the certificate of the single ADMM solvers (include/slp_hip_ext_admm_gap.h; ``ADMMState`` / ``_CGBase``
``.certificate`` / ``.set_stop_gap`` / ``.gap_state``, ``lp_admm_certified``, ``SparseLP.solve_admm_certified``): the repaired
multiplier gives a finite bound that never exceeds the HiGHS optimum on the oracle's iterates, a free original variable pushed
the wrong way gives ``-inf`` and never stops, the refusals come before the library is touched, and the prototypes sit in a header
of their own and are bound in a table of their own.  None of it needs a GPU."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

import admm_gap_cpu
import cp_gap_cpu
import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden, solver_args
from pysparselp_amd import _lib
from pysparselp_amd.ADMM import ADMMState, lp_admm, lp_admm_certified
from pysparselp_amd.admm_cg import ADMMCGLPState, ADMMCGState, DeviceADMM
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the list form)

GOLDENS = ("lp_potts8", "lp_random0", "lp_random1", "lp_random2", "lp_sc50a", "lp_sc105")
ITERATIONS, EVERY = 300, 10
HEADER = "slp_hip_ext_admm_gap.h"
NEW = sorted(["slp_admm_certificate", "slp_admm_cg_certificate", "slp_admm_set_stop_gap", "slp_admm_cg_set_stop_gap",
              "slp_admm_gap_state", "slp_admm_cg_gap_state", "slp_admm_cg_get_xp", "slp_admm_cg_get_lambda"])
PROTOTYPES = (
    "int slp_admm_certificate(slp_admm *s, double out[3]);",
    "int slp_admm_cg_certificate(slp_admm_cg *s, double out[3]);",
    "int slp_admm_set_stop_gap(slp_admm *s, double tol_gap, double tol_feas, int64_t check_every);",
    "int slp_admm_cg_set_stop_gap(slp_admm_cg *s, double tol_gap, double tol_feas, int64_t check_every);",
    "int slp_admm_gap_state(slp_admm *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);",
    "int slp_admm_cg_gap_state(slp_admm_cg *s, int64_t *iterations, int32_t *stopped, double *primal, double *bound, double *violation);",
    "int slp_admm_cg_get_xp(slp_admm_cg *s, double *xp, int64_t count);",
    "int slp_admm_cg_get_lambda(slp_admm_cg *s, double *lam);",
)


@functools.lru_cache(maxsize=None)
def problem_of(name):
    return solver_args(load_golden(name))


@functools.lru_cache(maxsize=None)
def numbers_of(name):
    """``{t: admm_gap_cpu.Numbers}`` at every 10th of 300 oracle iterations (shared, read only)."""
    p = problem_of(name)
    r = admm_gap_cpu.Restatement(admm_gap_cpu.setup_of(p))
    return {t: r.at(x, lam) for t, (x, lam) in admm_gap_cpu.iterates(p, ITERATIONS, EVERY).items()}


@pytest.mark.parametrize("name", GOLDENS)
def test_the_repaired_bound_is_finite_and_below_the_optimum(name):
    p = problem_of(name)
    n = np.asarray(p[0]).size
    # the original variables are boxed: no check below is left out for an infinite bound (cap on left-out cases: zero)
    assert np.all(np.isfinite(p[6])) and np.all(np.isfinite(p[7])) and np.asarray(p[6]).size == n
    res = cp_gap_cpu.highs_optimum(p)
    assert res.status == 0
    numbers = numbers_of(name)
    assert sorted(numbers) == list(range(EVERY, ITERATIONS + 1, EVERY))
    slack = admm_gap_cpu.HIGHS_SLACK * (1.0 + abs(res.fun))   # HiGHS's own accuracy: not a derived figure (admm_gap_cpu)
    for t, nb in numbers.items():
        assert np.isfinite(nb.bound), t
        assert nb.bound <= res.fun + nb.tol_bound + slack, (t, nb.bound, res.fun)
        assert nb.violation >= 0.0 and np.isfinite(nb.primal)
    if name != "lp_sc105":
        assert sum(nb.repaired for nb in numbers.values()) >= 1


def test_without_the_repair_a_repaired_check_has_no_bound():
    from oracle import oracle

    p = problem_of("lp_random0")
    r = admm_gap_cpu.Restatement(admm_gap_cpu.setup_of(p))
    seen = 0
    for x, lam in admm_gap_cpu.iterates(p, 60, EVERY).values():
        if r.yhat(lam)[1]:
            seen += 1
            with np.errstate(invalid="ignore", over="ignore"):
                d = r.c + oracle.rmatvec(r.a, lam)   # the multiplier as it stands
                terms = np.where(d != 0, np.minimum(d * r.lb, d * r.ub), 0.0)
            assert np.sum(terms) == -np.inf and np.isfinite(r.at(x, lam).bound)
    assert seen >= 1


def test_a_free_variable_pushed_the_wrong_way_gives_no_bound_and_never_stops():
    # minimise x0 + x1 with x0 free, x0 + x1 <= 4, x0 - x1 = 0: at lam = 0, d_0 = c_0 = 1 > 0 pushes x0 to its missing lower bound
    c = np.array([1.0, 1.0])
    a_eq, beq = scipy.sparse.csr_matrix(np.array([[1.0, -1.0]])), np.zeros(1)
    a_in, bu = scipy.sparse.csr_matrix(np.array([[1.0, 1.0]])), np.array([4.0])
    lb, ub = np.array([-np.inf, -1.0]), np.array([np.inf, 5.0])
    p = (c, a_eq, beq, a_in, None, bu, lb, ub)
    r = admm_gap_cpu.Restatement(admm_gap_cpu.setup_of(p))
    nb = r.at(np.zeros(r.N), np.zeros(r.m))
    assert nb.bound == -np.inf and nb.repaired == 0
    assert not admm_gap_cpu.decision(nb.primal, nb.bound, 0.0, 1e300, 1e300)
    for x, lam in admm_gap_cpu.iterates(p, 40, 10).values():
        nb = r.at(x, lam)
        if nb.bound == -np.inf:
            assert not admm_gap_cpu.decision(nb.primal, nb.bound, nb.violation, 1e300, 1e300)


def test_a_bad_tolerance_or_cadence_is_refused_before_the_library(no_library):  # noqa: F811
    p = problem_of("lp_random1")
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    with pytest.raises(ValueError, match="tol_gap must be a finite float >= 0"):
        lp_admm_certified(*p, tol_gap=-1, tol_feas=1e-2)
    with pytest.raises(ValueError, match="check_every must be an int >= 1"):
        lp_admm_certified(*p, tol_gap=1e-2, tol_feas=1e-2, check_every=0)
    for xstep in ("gauss_seidel", "cg", "auto"):
        for tol in BAD_TOL:
            for name, args in (("tol_gap", (tol, 1e-2)), ("tol_feas", (1e-2, tol))):
                match = f"{name} must be a finite float >= 0"
                with pytest.raises(ValueError, match=match):
                    lp_admm_certified(*p, *args, xstep=xstep)
                with pytest.raises(ValueError, match=match):
                    lp.solve_admm_certified(*args, xstep=xstep)
        for every in BAD_EVERY:
            with pytest.raises(ValueError, match="check_every must be an int >= 1"):
                lp_admm_certified(*p, 1e-2, 1e-2, every, xstep=xstep)
            with pytest.raises(ValueError, match="check_every must be an int >= 1"):
                lp.solve_admm_certified(1e-2, 1e-2, check_every=every, xstep=xstep)
    with pytest.raises(ValueError, match="unknown xstep"):
        lp.solve_admm_certified(1e-2, 1e-2, xstep="jacobi")
    for cls in (ADMMState, ADMMCGState, ADMMCGLPState, DeviceADMM):
        st = cls.__new__(cls)   # a state without a device: set_stop_gap must refuse before it looks for one
        with pytest.raises(ValueError, match="tol_feas must be a finite float >= 0"):
            st.set_stop_gap(1e-2, -1.0)
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            st.set_stop_gap(1e-2, 1e-2, 0)
    assert not hasattr(lp, "stop_info")


def test_an_accepted_call_gets_as_far_as_the_library(no_library):  # noqa: F811
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_admm_certified(*problem_of("lp_random1"), 0.0, 0.0, 1, nb_iter=3)
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_from_golden(load_golden("lp_potts8"), SparseLP).solve_admm_certified(1e-2, 1e-2, nb_iter=3)


def test_names_and_signatures():
    assert "lp_admm_certified" in pysparselp_amd.__all__ and hasattr(pysparselp_amd, "lp_admm_certified")
    assert "lp_admm_certified" in pysparselp_amd.__doc__ and len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    assert str(inspect.signature(lp_admm_certified)) == (
        "(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_gap, tol_feas, check_every=10, x0=None, gamma_eq=2, gamma_ineq=3, "
        "nb_iter=100, callback_func=None, max_time=None, use_preconditioning=True, nb_iter_plot=10, order=0, xstep='gauss_seidel', "
        "setup='auto')")
    assert list(inspect.signature(SparseLP.solve_admm_certified).parameters)[:5] == ["self", "tol_gap", "tol_feas", "check_every", "xstep"]
    for cls in (ADMMState, ADMMCGState, ADMMCGLPState, DeviceADMM):
        assert str(inspect.signature(cls.certificate)) == "(self)"
        assert str(inspect.signature(cls.set_stop_gap)) == "(self, tol_gap, tol_feas, check_every=1)"
        assert str(inspect.signature(cls.gap_state)) == "(self)"
        assert "row-normalised" in cls.certificate.__doc__
    for cls in (ADMMCGState, ADMMCGLPState, DeviceADMM):
        assert str(inspect.signature(cls.xp)) == "(self, count=None)" and str(inspect.signature(cls.lam)) == "(self)"
    assert "fixed_cost" in SparseLP.solve_admm_certified.__doc__ and "row-normalised" in SparseLP.solve_admm_certified.__doc__
    # solve and lp_admm keep their signatures
    assert list(inspect.signature(SparseLP.solve).parameters)[:5] == ["self", "method", "get_timing", "x0", "nb_iter"]
    assert list(inspect.signature(lp_admm).parameters)[-3:] == ["order", "xstep", "setup"]


def _strip(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_prototypes_are_in_a_header_of_their_own_and_bound():
    include = os.path.join(REPO, "include")
    assert f'#include "{HEADER}"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    raw = open(os.path.join(include, HEADER)).read()
    assert "row-normalised units" in raw
    ext = _strip(raw)
    for prototype in PROTOTYPES:
        assert prototype in ext, prototype
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_ADMM_GAP_SYMBOLS) == NEW
    assert _lib.EXT_ADMM_GAP_SYMBOLS == tuple(_lib._EXT_ADMM_GAP_SIGNATURES)
    for other in sorted(os.listdir(include)):   # ... and in no other header
        if other != HEADER:
            text = _strip(open(os.path.join(include, other)).read())
            assert not any(re.search(r"\b" + name + r"\b", text) for name in NEW), other
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert name not in _lib.EXPORTED_SYMBOLS and name not in _lib.EXT_CP_GAP_SYMBOLS
        assert getattr(lib, name).restype is _lib.c_int
    readme = open(os.path.join(REPO, "README.md")).read()
    assert HEADER in readme and all(name in readme for name in NEW)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/" + HEADER) == 2 and makefile.count("slp_gap_fold.h") == 2 and makefile.count(" slp_admm_gap.h") == 2


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    out = np.zeros(3)
    for prefix in ("slp_admm", "slp_admm_cg"):
        assert getattr(lib, prefix + "_certificate")(None, _lib.ptr(out)) != 0
        assert getattr(lib, prefix + "_set_stop_gap")(None, 1e-2, 1e-2, 1) != 0 and b"NULL handle" in lib.slp_last_error()
        assert getattr(lib, prefix + "_gap_state")(None, None, None, None, None, None) != 0 and b"NULL handle" in lib.slp_last_error()
    assert lib.slp_admm_cg_get_xp(None, _lib.ptr(out), 1) != 0 and lib.slp_admm_cg_get_lambda(None, _lib.ptr(out)) != 0
