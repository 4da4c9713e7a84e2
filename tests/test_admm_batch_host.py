"""Host logic of the batched ADMM (``lp_admm_batch``, ``SparseLP.solve_admm_batch``): every shape, finiteness and column-index
error is raised before the library is loaded.  None of it needs a GPU."""
import numpy as np
import pytest
import scipy.sparse

from conftest import lp_from_golden, load_golden, solver_args
from pysparselp_amd import _lib, lp_admm_batch
from pysparselp_amd.SparseLP import SparseLP


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load or bind the library fails the test: validation must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _lp(batch=3):
    d = load_golden("lp_random1")
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = solver_args(d)
    cs = np.tile(c, (batch, 1)) + np.random.RandomState(0).randn(batch, c.size)
    return cs, a_eq, beq, a_ineq, bl, bu, lb, ub


def test_shapes_of_the_costs_are_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    with pytest.raises(ValueError, match=r"expected \(B, n\)"):
        lp_admm_batch(cs[0], a_eq, beq, a_ineq, bl, bu, lb, ub)
    with pytest.raises(ValueError, match="columns"):
        lp_admm_batch(cs[:, :-1], a_eq, beq, a_ineq, bl, bu, lb[:-1], ub[:-1])
    with pytest.raises(ValueError, match="B >= 1"):
        lp_admm_batch(cs[:0], a_eq, beq, a_ineq, bl, bu, lb, ub)


def test_wrong_leading_axis_of_bounds_and_start_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    n = cs.shape[1]
    with pytest.raises(ValueError, match="lb has shape"):
        lp_admm_batch(cs, a_eq, beq, a_ineq, bl, bu, np.tile(lb, (2, 1)), ub)
    with pytest.raises(ValueError, match="ub has shape"):
        lp_admm_batch(cs, a_eq, beq, a_ineq, bl, bu, lb, ub[:-1])
    with pytest.raises(ValueError, match="x0 has shape"):
        lp_admm_batch(cs, a_eq, beq, a_ineq, bl, bu, lb, ub, x0=np.zeros((3, n + 1)))


@pytest.mark.parametrize("which", ["beq", "b_lower", "b_upper"])
def test_per_instance_right_hand_sides_are_refused(no_library, which):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    rhs = dict(beq=beq, b_lower=bl, b_upper=bu)
    rhs[which] = np.tile(rhs[which], (3, 1))
    with pytest.raises(ValueError, match=which + " has shape .*not built"):
        lp_admm_batch(cs, a_eq, rhs["beq"], a_ineq, rhs["b_lower"], rhs["b_upper"], lb, ub)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_cost_that_is_not_finite_is_refused(no_library, bad):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    cs[2, 4] = bad
    with pytest.raises(ValueError, match="instance 2 .*not finite"):
        lp_admm_batch(cs, a_eq, beq, a_ineq, bl, bu, lb, ub)


@pytest.mark.parametrize("block", ["a_eq", "a_ineq"])
def test_column_index_out_of_range_is_refused(no_library, block):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(2)
    n = cs.shape[1]
    mats = dict(a_eq=a_eq, a_ineq=a_ineq)
    bad = scipy.sparse.csr_matrix(mats[block])
    bad.indices = bad.indices.copy()
    bad.indices[3] = n   # first index past the end
    assert bad.shape[1] == n
    mats[block] = bad
    with pytest.raises(ValueError, match=block + " has a column index outside"):
        lp_admm_batch(cs, mats["a_eq"], beq, mats["a_ineq"], bl, bu, lb, ub)


def test_a_missing_inequality_block_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(2)
    with pytest.raises(ValueError, match="no inequality block"):
        lp_admm_batch(cs, a_eq, beq, None, None, None, lb, ub)


def test_solve_admm_batch_validates_before_loading(no_library):
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    n = lp.nb_variables
    costs = np.tile(lp.costsvector, (2, 1))
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_admm_batch(costs[:, :-1])
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_admm_batch(costs[0])
    with pytest.raises(ValueError, match="B >= 1"):
        lp.solve_admm_batch(np.zeros((0, n)))
    costs[1, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        lp.solve_admm_batch(costs)
    # an LP without inequality rows: the standard form of the reference does not exist (tools.py:92)
    eq_only = lp_from_golden(load_golden("lp_sc105"), SparseLP)
    eq_only.a_inequalities = scipy.sparse.csr_matrix((0, eq_only.nb_variables))
    eq_only.b_upper, eq_only.b_lower = np.zeros(0), None
    with pytest.raises(ValueError, match="no inequality block"):
        eq_only.solve_admm_batch(np.tile(eq_only.costsvector, (2, 1)))


def test_solve_batch_still_refuses_admm(no_library):
    """``solve_batch`` is the batched Chambolle-Pock only; the batched ADMM is a method of its own."""
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    costs = np.tile(lp.costsvector, (2, 1))
    with pytest.raises(ValueError, match="chambolle_pock_ppd"):
        lp.solve_batch(costs, method="admm")


def test_the_bindings_declare_the_batched_entry_points():
    names = ["create_lp", "destroy", "iterate", "sweep_step", "multiplier_step", "report", "get_x", "get_lambda", "num_levels", "form",
             "bench"]
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_admm_batch_")) == sorted("slp_admm_batch_" + n for n in names)
