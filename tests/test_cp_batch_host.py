"""Host logic of the batched Chambolle-Pock (``chambolle_pock_ppd_batch``, ``SparseLP.solve_batch``): argument validation,
the no-constraint case and the batched one-sided stacking.  None of it loads the library or needs a GPU."""
import numpy as np
import pytest
import scipy.sparse

from conftest import lp_from_golden, load_golden, solver_args
from pysparselp_amd import _lib, chambolle_pock_ppd_batch
from pysparselp_amd.ChambollePockPPD import one_sided_system, one_sided_system_batch
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


def test_wrong_leading_axis_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    n, rows = cs.shape[1], a_ineq.shape[0]
    with pytest.raises(ValueError, match="lb has shape"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, bl, bu, np.tile(lb, (2, 1)), ub)
    with pytest.raises(ValueError, match="ub has shape"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, bl, bu, lb, ub[:-1])
    with pytest.raises(ValueError, match="b_upper has shape"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, bl, np.zeros((4, rows)), lb, ub)
    with pytest.raises(ValueError, match="x0 has shape"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, bl, bu, lb, ub, x0=np.zeros((3, n + 1)))
    with pytest.raises(ValueError, match=r"expected \(B, n\)"):
        chambolle_pock_ppd_batch(cs[0], a_eq, beq, a_ineq, bl, bu, lb, ub)
    if a_eq is not None:
        with pytest.raises(ValueError, match="beq has shape"):
            chambolle_pock_ppd_batch(cs, a_eq, np.zeros((2, a_eq.shape[0])), a_ineq, bl, bu, lb, ub)


def test_empty_batch_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    with pytest.raises(ValueError, match="B >= 1"):
        chambolle_pock_ppd_batch(cs[:0], a_eq, beq, a_ineq, bl, bu, lb, ub)


def test_finite_pattern_mismatch_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(3)
    rows = a_ineq.shape[0]
    bus = np.tile(bu, (3, 1))
    bus[2, 1] = np.inf   # instance 2 lacks a row the others have
    with pytest.raises(ValueError, match="instance 2 .*pattern"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, np.full(rows, -np.inf), bus, lb, ub)
    bls = np.full((3, rows), -np.inf)
    bls[1, 0] = bu[0] - 1.0   # instance 1 has a lower-bounded row of its own
    with pytest.raises(ValueError, match="instance 1 .*pattern"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, a_ineq, bls, bu, lb, ub)


def test_column_index_out_of_range_is_refused(no_library):
    cs, a_eq, beq, a_ineq, bl, bu, lb, ub = _lp(2)
    n = cs.shape[1]
    bad = scipy.sparse.csr_matrix(a_ineq)
    bad.indices = bad.indices.copy()
    bad.indices[3] = n   # first index past the end
    assert bad.shape[1] == n
    with pytest.raises(ValueError, match="column index outside"):
        chambolle_pock_ppd_batch(cs, a_eq, beq, bad, bl, bu, lb, ub)


def test_solve_batch_validates_before_loading(no_library):
    lp = lp_from_golden(load_golden("lp_potts8"), SparseLP)
    n = lp.nb_variables
    costs = np.tile(lp.costsvector, (2, 1))
    for method in ("admm", "admm2", "dual_gradient_ascent", "nonsense"):
        with pytest.raises(ValueError, match="chambolle_pock_ppd"):
            lp.solve_batch(costs, method=method)
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_batch(costs[:, :-1])
    with pytest.raises(ValueError, match="costs has shape"):
        lp.solve_batch(costs[0])
    with pytest.raises(ValueError, match="B >= 1"):
        lp.solve_batch(np.zeros((0, n)))


def test_no_constraints_gives_the_box_vertex_per_instance(no_library):
    rng = np.random.RandomState(5)
    n, batch = 7, 4
    c = rng.randn(batch, n)
    c[1, 2] = 0.0
    lb, ub = -rng.rand(n) - 1, rng.rand(n) + 1
    x = chambolle_pock_ppd_batch(c, None, None, None, None, None, lb, ub)
    want = np.where(c > 0, lb, np.where(c < 0, ub, 0.0))
    assert x.shape == (batch, n) and np.array_equal(x, want)
    # per-instance bounds, empty matrices instead of None (reference :70-72)
    lbs, ubs = np.tile(lb, (batch, 1)) - rng.rand(batch, n), np.tile(ub, (batch, 1)) + rng.rand(batch, n)
    empty = scipy.sparse.csr_matrix((0, n))
    x = chambolle_pock_ppd_batch(c, empty, np.zeros(0), empty, None, np.zeros(0), lbs, ubs)
    assert np.array_equal(x, np.where(c > 0, lbs, np.where(c < 0, ubs, 0.0)))
    # each row is what the single-instance rule gives (:147-151)
    for k in range(batch):
        one = np.zeros(n)
        one[c[k] > 0] = lbs[k][c[k] > 0]
        one[c[k] < 0] = ubs[k][c[k] < 0]
        assert np.array_equal(x[k], one)


@pytest.mark.parametrize("form", ["two_sided", "lower_only", "upper_only", "no_lower", "shared"])
def test_batched_one_sided_stacking_equals_the_single_instance_one(form):
    rng = np.random.RandomState(11)
    rows, n, batch = 9, 6, 4
    a = scipy.sparse.random(rows, n, density=0.5, random_state=rng, format="csr")
    a.data = rng.randn(a.nnz)
    bu = rng.randn(batch, rows) + 2
    bl = bu - 1 - rng.rand(batch, rows)
    if form == "two_sided":   # some rows upper only, some lower only, some both
        bu[:, [0, 4]] = np.inf
        bl[:, [1, 4, 7]] = -np.inf
    elif form == "lower_only":
        bu[:] = np.inf
    elif form == "upper_only":
        bl[:] = -np.inf
    elif form == "no_lower":
        bl = None
        bu[:, 2] = np.inf   # stays, as in the reference: without b_lower no row is selected
    elif form == "shared":
        bu, bl = bu[0], bl[0]
        bu[3] = np.inf
    mat, b = one_sided_system_batch(a, bl, bu)
    if form == "shared":
        ref_mat, ref_b = one_sided_system(a, bl, bu)
        assert b.shape == ref_b.shape and np.array_equal(b, ref_b)
        for got, want in zip(mat[:3], ref_mat[:3]):
            assert np.array_equal(got, want)
        return
    assert b.shape == (batch, mat[3])
    for k in range(batch):
        ref_mat, ref_b = one_sided_system(a, None if bl is None else bl[k], bu[k])
        assert mat[3] == ref_mat[3]
        for got, want in zip(mat[:3], ref_mat[:3]):
            assert np.array_equal(got, want)
        assert np.array_equal(b[k], ref_b)
    # one bound shared, the other per instance
    if form == "two_sided":
        mat2, b2 = one_sided_system_batch(a, bl[0], bu)
        for k in range(batch):
            ref_mat, ref_b = one_sided_system(a, bl[0], bu[k])
            assert np.array_equal(b2[k], ref_b) and np.array_equal(mat2[2], ref_mat[2])
