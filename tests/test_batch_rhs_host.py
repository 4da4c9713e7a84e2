"""Host side of per-instance right-hand sides for the batched dual gradient ascent and the batched ADMM solver
(``slp_batch_dga_set_rhs`` / ``slp_admm_batch_set_rhs``; ``DeviceDGABatch.set_rhs``, ``ADMMBatchState.set_rhs``,
``dual_gradient_ascent_batch_rhs``, ``lp_admm_batch_rhs``, ``SparseLP.solve_dga_batch_rhs`` / ``solve_admm_batch_rhs``): the two
prototypes are in a header of their own and bound in a table of their own while slp_hip.h and its 215 entry points stay, the
signatures are the announced ones, and every refusal comes before the library is touched.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import pysparselp_amd
from conftest import REPO, load_golden, solver_args
from dga_batch_cases import batch_case
from dga_many_cases import LP
from pysparselp_amd import ADMMBatchState, DeviceDGABatch, _lib, dual_gradient_ascent_batch_rhs, lp_admm_batch_rhs
from pysparselp_amd.SparseLP import SparseLP
from test_cp_many_stop_host import BAD_EVERY, BAD_TOL, no_library  # noqa: F401  (the fixture and the two lists of the CP form)

NEW = ["slp_admm_batch_set_rhs", "slp_batch_dga_set_rhs"]
HEADER = "slp_hip_ext_batch_rhs.h"
PROTOTYPES = (
    "int slp_batch_dga_set_rhs(slp_batch_dga *s, const double *b, int b_batched);",
    "int slp_admm_batch_set_rhs(slp_admm_batch *s, const double *b_eq, int b_eq_batched, const double *b_lower, int b_lower_batched, "
    "const double *b_upper, int b_upper_batched);",
)


def _strip(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_two_prototypes_are_in_a_header_of_their_own_and_bound():
    include = os.path.join(REPO, "include")
    assert f'#include "{HEADER}"' in open(os.path.join(include, "slp_hip_ext.h")).read()
    ext = _strip(open(os.path.join(include, HEADER)).read())
    for prototype in PROTOTYPES:
        assert prototype in ext, prototype
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", ext)))
    assert declared == sorted(_lib.EXT_BATCH_RHS_SYMBOLS) == NEW
    assert _lib.EXT_BATCH_RHS_SYMBOLS == tuple(_lib._EXT_BATCH_RHS_SIGNATURES)
    for other in sorted(os.listdir(include)):   # ... and in no other header
        if other != HEADER:
            text = _strip(open(os.path.join(include, other)).read())
            assert not any(name in text for name in NEW), other
    assert len(_lib.EXPORTED_SYMBOLS) == 215
    others = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.EXT_ADMM_BATCH_SYMBOLS, _lib.EXT_DGA_BATCH_SYMBOLS, _lib.EXT_DGA_MANY_SYMBOLS,
              _lib.EXT_DGA_MANY_LIVE_SYMBOLS, _lib.EXT_MANY_LIVE_SYMBOLS, _lib.EXT_TALL_SYMBOLS)
    lib = _lib.load()   # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
        assert all(name not in table for table in others), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.c_int
    assert lib.slp_batch_dga_set_rhs.argtypes == [_lib.c_vp, _lib.c_vp, _lib.c_int]
    assert lib.slp_admm_batch_set_rhs.argtypes == [_lib.c_vp] + [_lib.c_vp, _lib.c_int] * 3
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "C ABI (215 entry points)" in readme and HEADER in readme and all(name in readme for name in NEW)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert makefile.count("../../include/" + HEADER) == 2   # both dependency lists


def test_the_signatures_are_the_announced_ones():
    assert str(inspect.signature(dual_gradient_ascent_batch_rhs)) == (
        "(lp, costs, b_equalities=None, b_upper=None, tol=None, targets=None, check_every=10, nb_max_iter=1000, callback_func=None, "
        "y_eq=None, y_ineq=None, max_time=None, lower_bounds=None, upper_bounds=None, path=None)")
    assert str(inspect.signature(lp_admm_batch_rhs)) == (
        "(cs, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, tol_residual=None, tol_step=None, check_every=10, x0=None, gamma_eq=2, "
        "gamma_ineq=3, nb_iter=100, callback_func=None, max_time=None, use_preconditioning=True, nb_iter_plot=10)")
    assert str(inspect.signature(DeviceDGABatch.set_rhs)) == "(self, b)"
    assert str(inspect.signature(ADMMBatchState.set_rhs)) == "(self, beq=None, b_lower=None, b_upper=None)"
    dga = list(inspect.signature(SparseLP.solve_dga_batch_rhs).parameters)
    assert dga[:7] == ["self", "costs", "b_equalities", "b_upper", "tol", "targets", "check_every"]
    assert dga[7:] == list(inspect.signature(SparseLP.solve_dga_batch_until).parameters)[5:]
    admm = list(inspect.signature(SparseLP.solve_admm_batch_rhs).parameters)
    assert admm[:8] == ["self", "costs", "b_equalities", "b_lower", "b_upper", "tol_residual", "tol_step", "check_every"]
    assert admm[8:] == list(inspect.signature(SparseLP.solve_admm_batch_until).parameters)[5:]
    for name in ("tol", "targets"):
        assert inspect.signature(SparseLP.solve_dga_batch_rhs).parameters[name].default is None
    for name in ("tol_residual", "tol_step"):
        assert inspect.signature(SparseLP.solve_admm_batch_rhs).parameters[name].default is None
    for name in ("dual_gradient_ascent_batch_rhs", "lp_admm_batch_rhs"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name) and name in pysparselp_amd.__doc__, name
    for name in ("solve_dga_batch_rhs", "solve_admm_batch_rhs", "set_rhs"):
        assert name in pysparselp_amd.__doc__, name
    assert len(set(pysparselp_amd.__all__)) == len(pysparselp_amd.__all__)
    # the old functions point to the new ones instead of saying that the capability does not exist
    for fn, new in ((pysparselp_amd.lp_admm_batch, "lp_admm_batch_rhs"), (pysparselp_amd.dual_gradient_ascent_batch, "dual_gradient_ascent_batch_rhs")):
        assert new in fn.__doc__ and "not built" not in fn.__doc__


# ---------------------------------------------------------------------------------------------------------------- dual ascent
B = 4


def _dga():
    args, six = batch_case("sc50a")
    c, a_eq, b_eq, a_ineq, b_upper, lb, ub = args
    return LP(c, a_eq, b_eq, a_ineq, b_upper, lb, ub), six[:B], a_eq.shape[0], a_ineq.shape[0]


class _NoDGA(DeviceDGABatch):
    """A state without a device: ``set_rhs`` must refuse before it looks for one."""

    def __init__(self, batch, m):
        self.batch, self.m, self._h = batch, m, None


def test_dga_right_hand_sides_are_checked_before_the_library(no_library):
    lp, costs, m_eq, m_in = _dga()
    be, bu = np.tile(lp.b_equalities, (B, 1)), np.tile(lp.b_upper, (B, 1))
    for kw in (dict(b_equalities=be[:B - 1]), dict(b_upper=bu[:B - 1]), dict(b_equalities=be[:, :-1]), dict(b_upper=bu[0, :-1]),
               dict(b_equalities=be[None])):
        with pytest.raises(ValueError, match=r"has shape .*expected \(\d+,\) shared by the instances, or \(B, \d+\) with B = 4"):
            dual_gradient_ascent_batch_rhs(lp, costs, **kw)
    bad = bu.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="b_upper has a NaN"):
        dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bad)
    nan1 = lp.b_equalities.copy()
    nan1[0] = np.nan
    with pytest.raises(ValueError, match="b_equalities has a NaN"):
        dual_gradient_ascent_batch_rhs(lp, costs, b_equalities=nan1)
    for value in (np.inf, -np.inf):
        bad = bu.copy()
        bad[2, 3] = value
        with pytest.raises(ValueError, match="instance 2 has an entry of b_upper that is not finite"):
            dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bad)
        bad = be.copy()
        bad[3, 0] = value
        with pytest.raises(ValueError, match="instance 3 has an entry of b_equalities that is not finite"):
            dual_gradient_ascent_batch_rhs(lp, costs, b_equalities=bad)
    # the stopping arguments are those of dual_gradient_ascent_batch_until
    for tol in BAD_TOL:
        if tol is not None:   # None: no step test
            with pytest.raises(ValueError, match="tol must be a finite float >= 0"):
                dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bu, tol=tol)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bu, tol=1e-3, check_every=every)
    with pytest.raises(ValueError, match="targets"):
        dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bu, targets=np.zeros(B + 1))
    with pytest.raises(ValueError, match="targets holds a NaN or -inf"):
        dual_gradient_ascent_batch_rhs(lp, costs, b_upper=bu, targets=-np.inf)
    # a finite b_lower is refused as by the other forms
    two = LP(lp.costsvector, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
    two.b_lower = np.zeros(m_in)
    with pytest.raises(ValueError, match="one-sided"):
        dual_gradient_ascent_batch_rhs(two, costs, b_upper=bu)
    with pytest.raises(ValueError, match=r"costs has shape"):
        dual_gradient_ascent_batch_rhs(lp, costs[0], b_upper=bu)
    # SparseLP: the same checks, before the curves are touched
    slp = SparseLP.__new__(SparseLP)
    slp.__dict__.update(nb_variables=costs.shape[1], costsvector=lp.costsvector, a_equalities=lp.a_equalities, b_equalities=lp.b_equalities,
                        a_inequalities=lp.a_inequalities, b_upper=lp.b_upper, b_lower=None, lower_bounds=lp.lower_bounds,
                        upper_bounds=lp.upper_bounds, itrn_curve="untouched")
    with pytest.raises(ValueError, match="instance 1 has an entry of b_upper that is not finite"):
        bad = bu.copy()
        bad[1, 0] = np.inf
        slp.solve_dga_batch_rhs(costs, b_upper=bad)
    with pytest.raises(ValueError, match="has shape"):
        slp.solve_dga_batch_rhs(costs, b_equalities=be[:B - 1])
    assert slp.itrn_curve == "untouched"


def test_dga_state_set_rhs_is_checked_before_the_library(no_library):
    state = _NoDGA(batch=3, m=5)
    for bad in (np.zeros(4), np.zeros((2, 5)), np.zeros((3, 4)), np.zeros((1, 3, 5)), 1.0):
        with pytest.raises(ValueError, match="b has shape"):
            state.set_rhs(bad)
    for shape in ((5,), (3, 5)):
        b = np.zeros(shape)
        b[-1] = np.nan
        with pytest.raises(ValueError, match="b has a NaN"):
            state.set_rhs(b)
    b = np.zeros((3, 5))
    b[1, 4] = np.inf
    with pytest.raises(ValueError, match="instance 1 has an entry of b that is not finite"):
        state.set_rhs(b)


# ---------------------------------------------------------------------------------------------------------------- ADMM
def _admm():
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = solver_args(load_golden("lp_random1"))
    rs = np.random.RandomState(2)
    cs = c * (1 + 0.1 * rs.rand(B, c.size))
    bl = np.where(np.isfinite(bu), bu - 1.0, -np.inf)   # a two-sided block, whatever the fixture has
    return cs, a_eq, beq, a_ineq, bl, bu, lb, ub


class _NoADMM(ADMMBatchState):
    def __init__(self, batch, m_eq, m_ineq, b_lower=None, b_upper=None):
        self.batch, self.m_eq, self.m_ineq, self._b_lower, self._b_upper, self._h = batch, m_eq, m_ineq, b_lower, b_upper, None


def test_admm_right_hand_sides_are_checked_before_the_library(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _admm()
    beqs, bls, bus = (np.tile(v, (B, 1)) for v in (beq, bl, bu))
    run = lambda beq=beq, bl=bl, bu=bu, **kw: lp_admm_batch_rhs(cs, a_eq, beq, a_ineq, bl, bu, lb, ub, **kw)  # noqa: E731
    for kw in (dict(beq=beqs[:B - 1]), dict(bl=bls[:B - 1]), dict(bu=bus[:B - 1]), dict(beq=beqs[:, :-1]), dict(bl=bl[:-1]),
               dict(bu=bus[:, 1:]), dict(bu=bus[None])):
        with pytest.raises(ValueError, match=r"has shape .*expected \(\d+,\) shared by the instances, or \(B, \d+\) with B = 4"):
            run(**kw)
    for name, key, arr in (("beq", "beq", beqs), ("b_lower", "bl", bls), ("b_upper", "bu", bus)):
        bad = arr.copy()
        bad[1, 0] = np.nan
        with pytest.raises(ValueError, match=f"{name} has a NaN"):
            run(**{key: bad})
    bad = beqs.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="instance 2 has an entry of beq that is not finite"):
        run(beq=bad)
    row = int(np.flatnonzero(np.isfinite(bu))[0])
    crossed = bls.copy()
    crossed[3, row] = bu[row] + 1.0
    with pytest.raises(ValueError, match=f"instance 3 has b_lower > b_upper on row {row}"):
        run(bl=crossed)
    crossed = bus.copy()
    crossed[1, row] = bl[row] - 0.5
    with pytest.raises(ValueError, match=f"instance 1 has b_lower > b_upper on row {row}"):
        run(bu=crossed)
    equal = bls.copy()
    equal[3, row] = bu[row]   # b_lower == b_upper is no error: the call gets as far as the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        run(bl=equal)
    # the stopping arguments are those of lp_admm_batch_until, and the two tolerances go together
    for tol in BAD_TOL:
        if tol is not None:
            with pytest.raises(ValueError, match="tol_residual must be a finite float >= 0"):
                run(bu=bus, tol_residual=tol, tol_step=1e-3)
            with pytest.raises(ValueError, match="tol_step must be a finite float >= 0"):
                run(bu=bus, tol_residual=1e-3, tol_step=tol)
    for every in BAD_EVERY:
        with pytest.raises(ValueError, match="check_every must be an int >= 1"):
            run(bu=bus, tol_residual=1e-3, tol_step=1e-3, check_every=every)
    for kw in (dict(tol_residual=1e-3), dict(tol_step=1e-3)):
        with pytest.raises(ValueError, match="tol_residual and tol_step go together"):
            run(bu=bus, **kw)
    # what lp_admm_batch refuses stays refused
    with pytest.raises(ValueError, match="cs has shape"):
        lp_admm_batch_rhs(cs[0], a_eq, beq, a_ineq, bl, bus, lb, ub)
    with pytest.raises(ValueError, match="no inequality block"):
        lp_admm_batch_rhs(cs, a_eq, beqs, None, None, None, lb, ub)
    with pytest.raises(ValueError, match="lb has shape"):
        lp_admm_batch_rhs(cs, a_eq, beqs, a_ineq, bl, bu, lb[:-1], ub)


def test_admm_state_set_rhs_is_checked_before_the_library(no_library):
    lo, hi = np.array([0.0, -np.inf, 1.0]), np.array([1.0, 2.0, np.inf])
    state = _NoADMM(batch=2, m_eq=4, m_ineq=3, b_lower=lo, b_upper=hi)
    for kw in (dict(beq=np.zeros(3)), dict(beq=np.zeros((3, 4))), dict(b_lower=np.zeros(4)), dict(b_upper=np.zeros((1, 3)))):
        with pytest.raises(ValueError, match="has shape"):
            state.set_rhs(**kw)
    with pytest.raises(ValueError, match="b_upper has a NaN"):
        state.set_rhs(b_upper=np.array([1.0, np.nan, 2.0]))
    with pytest.raises(ValueError, match="instance 1 has an entry of beq that is not finite"):
        state.set_rhs(beq=np.array([[0.0] * 4, [0.0, -np.inf, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="beq has an entry that is not finite"):
        state.set_rhs(beq=np.array([0.0, np.inf, 0.0, 0.0]))
    # one side given: it is compared against the side the state keeps
    with pytest.raises(ValueError, match="instance 1 has b_lower > b_upper on row 0"):
        state.set_rhs(b_lower=np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="instance 0 has b_lower > b_upper on row 2"):
        state.set_rhs(b_upper=np.array([1.0, 1.0, 0.5]))
    with pytest.raises(ValueError, match="instance 0 has b_lower > b_upper on row 1"):
        state.set_rhs(b_lower=np.array([0.0, 3.0, 0.0]), b_upper=np.array([[1.0, 2.0, 3.0], [1.0, 4.0, 3.0]]))
    assert state._b_lower is lo and state._b_upper is hi   # a refusal changes nothing
    # infinite bounds of the inequality block are fine, and -inf < +inf is no crossing
    from pysparselp_amd.ADMM import _check_batch_rhs

    got = _check_batch_rhs(2, 4, 3, None, np.array([-np.inf, 0.0, -np.inf]), np.array([[np.inf, 0.0, 1.0], [np.inf, 1.0, 2.0]]))
    assert got[0] is None and got[1].shape == (3,) and got[2].shape == (2, 3)
    # a block without rows has no side
    assert _check_batch_rhs(2, 0, 3, np.zeros(0), None, None) == (None, None, None)


def test_admm_state_records_new_sides_only_when_the_library_accepted_them(monkeypatch):
    """After a refusal by the library (the state has iterated, or the memory does not fit) the C state keeps its sides, and so does
    what later calls are compared against."""
    from pysparselp_amd import SlpError

    class Lib:
        rc = 1

        def slp_admm_batch_set_rhs(self, *a):
            return self.rc

    monkeypatch.setattr(_lib, "last_error", lambda: "slp_admm_batch_set_rhs: the state has iterated")
    lo, hi = np.array([0.0, -np.inf, 1.0]), np.array([1.0, 2.0, np.inf])
    state = _NoADMM(batch=2, m_eq=0, m_ineq=3, b_lower=lo, b_upper=hi)
    state._l = Lib()
    new_lo, new_hi = np.array([[0.5, 0.0, 1.0], [0.0, 0.0, 0.0]]), np.array([2.0, 2.0, 3.0])
    with pytest.raises(SlpError, match="has iterated"):
        state.set_rhs(b_lower=new_lo, b_upper=new_hi)
    assert state._b_lower is lo and state._b_upper is hi
    state._l.rc = 0
    state.set_rhs(b_lower=new_lo, b_upper=new_hi)
    assert np.array_equal(state._b_lower, new_lo) and np.array_equal(state._b_upper, new_hi)
    with pytest.raises(ValueError, match="instance 0 has b_lower > b_upper on row 0"):
        state.set_rhs(b_upper=np.array([0.25, 2.0, 3.0]))   # against the new lower side 0.5
