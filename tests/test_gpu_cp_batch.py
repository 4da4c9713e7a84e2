"""Batched Chambolle-Pock (csrc/slp_cp_batch.hip, ``chambolle_pock_ppd_batch``, ``SparseLP.solve_batch``) on the GPU.

Every instance of a batch must be BIT FOR BIT the iterate of the reference (golden fixtures, the oracle) and of the shipped
single-instance solver in SEQUENTIAL order; the maxima of the report are exact, its two energies are sums in another order:
``rtol = atol = 1e-9``, the bar of ``test_gpu_parity.test_cp_iterates_bit_exact``.

Instances are built from the golden fixtures with seeded ``numpy.random.RandomState`` draws; instance 0 is always the fixture
itself.  Needs a real MI355X: run with ``-m gpu``.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest

from conftest import Recorder, lp_from_golden, load_golden
from oracle import oracle
from test_gpu_parity import CASES
from test_oracle_golden import _reduced

pytestmark = pytest.mark.gpu

ENERGY_TOL = dict(rtol=1e-9, atol=1e-9)
B_BASE = 5


def _mods():
    from pysparselp_amd import ORDER_SEQUENTIAL, CPBatchState, chambolle_pock_ppd_batch
    from pysparselp_amd.ChambollePockPPD import CPState, chambolle_pock_ppd, one_sided_system, one_sided_system_batch

    return CPBatchState, chambolle_pock_ppd_batch, CPState, chambolle_pock_ppd, one_sided_system, one_sided_system_batch, ORDER_SEQUENTIAL


class BatchRecorder:
    """Collects the callback calls of the batched solver at the iterations of ``keep`` (copies)."""

    def __init__(self, keep=None):
        self.keep = None if keep is None else set(int(k) for k in keep)
        self.it, self.x, self.e1, self.e2, self.veq, self.vineq = [], [], [], [], [], []

    def __call__(self, niter, sol, e1, e2, dur, veq, vineq):
        if self.keep is None or niter in self.keep:
            self.it.append(niter)
            for store, v in ((self.x, sol), (self.e1, e1), (self.e2, e2), (self.veq, veq), (self.vineq, vineq)):
                store.append(np.array(v, dtype=np.float64, copy=True))


def _instances(d, batch, seed, vary=("c",), two_sided=False):
    """The fixture's reduced LP as ``batch`` instances: a dict of the arguments of ``chambolle_pock_ppd_batch``.  ``vary`` names
    what differs between the instances (the others stay shared vectors); instance 0 is the fixture unperturbed."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = _reduced(d)
    if a_eq is not None and a_eq.shape[0] == 0:   # (the solver states take None for an absent kind of rows, reference :70-72)
        a_eq, beq = None, None
    rs = np.random.RandomState(seed)
    n = c.size
    cs = np.tile(c, (batch, 1))
    cs[1:] = c * (1 + 0.2 * rs.randn(batch - 1, n)) + 0.05 * np.mean(np.abs(c)) * rs.randn(batch - 1, n)
    args = dict(c=cs, a_eq=a_eq, beq=beq, a_ineq=a_ineq, b_lower=bl, b_upper=bu, lb=lb, ub=ub, x0=None)
    if two_sided:   # rows with both bounds, rows with a lower bound only, rows with an upper bound only
        rows = a_ineq.shape[0]
        bl2 = np.full(rows, -np.inf)
        bl2[0::3] = bu[0::3] - 1.5
        bu2 = bu.copy()
        bu2[0::6] = np.inf
        args["b_lower"], args["b_upper"] = bl2, bu2
    if "b" in vary:
        if a_eq is not None:
            bes = np.tile(beq, (batch, 1))
            bes[1:] += 0.01 * (1 + np.abs(beq)) * rs.randn(batch - 1, beq.size)
            args["beq"] = bes
        bus = np.tile(args["b_upper"], (batch, 1))
        bus[1:] += 0.01 * (1 + np.abs(np.where(np.isfinite(bus[1:]), bus[1:], 0))) * rs.rand(batch - 1, bus.shape[1])
        args["b_upper"] = bus
        if two_sided:
            bls = np.tile(args["b_lower"], (batch, 1))
            bls[1:] -= 0.01 * rs.rand(batch - 1, bls.shape[1])
            args["b_lower"] = bls
    if "bounds" in vary:   # widened per instance: lb <= ub is kept, infinite bounds stay infinite
        lbs, ubs = np.tile(lb, (batch, 1)), np.tile(ub, (batch, 1))
        lbs[1:] -= 0.1 * rs.rand(batch - 1, n)
        ubs[1:] += 0.1 * rs.rand(batch - 1, n)
        args["lb"], args["ub"] = lbs, ubs
    if "x0" in vary:
        x0 = np.zeros((batch, n))
        x0[1:] = 0.1 * rs.randn(batch - 1, n)
        args["x0"] = x0
    return args


def _of_instance(args, k):
    """The positional arguments (and x0) of a single-instance solver for instance ``k``."""
    pick = lambda v: v if (v is None or np.ndim(v) == 1) else v[k]  # noqa: E731
    return ((args["c"][k], args["a_eq"], pick(args["beq"]), args["a_ineq"], pick(args["b_lower"]), pick(args["b_upper"]),
             pick(args["lb"]), pick(args["ub"])), pick(args["x0"]))


def _run_batch(args, **kw):
    solve = _mods()[1]
    return solve(args["c"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"], args["ub"],
                 x0=args["x0"], **kw)


@functools.lru_cache(maxsize=None)
def _recorded(case, vary, two_sided=False):
    """One batched run of the fixture at its recorded iterations, shared by the tests that look at it (never modified)."""
    d = load_golden("lp_" + case)
    args = _instances(d, B_BASE, seed=len(case) + 17 * len(vary), vary=vary, two_sided=two_sided)
    rec = BatchRecorder(d["cp_it"])
    x, _ = _run_batch(args, nb_max_iter=int(d["cp_it"][-1]) + 1, callback_func=rec, nb_iter_plot=1)
    return d, args, rec, x


def _assert_instance_equals_oracle(d, args, rec, x_final, k):
    pos, x0 = _of_instance(args, k)
    ref = Recorder(d["cp_it"])
    xo, _ = oracle.chambolle_pock_ppd(*pos, x0=x0, nb_max_iter=int(d["cp_it"][-1]) + 1, callback_func=ref, nb_iter_plot=1)
    assert rec.it == ref.it
    assert np.array_equal(np.array(rec.x)[:, k], np.array(ref.x))
    assert np.array_equal(x_final[k], xo)
    assert np.array_equal(np.array(rec.veq)[:, k], np.asarray(ref.veq, dtype=np.float64))
    assert np.array_equal(np.array(rec.vineq)[:, k], np.asarray(ref.vineq, dtype=np.float64))
    np.testing.assert_allclose(np.array(rec.e1)[:, k], ref.e1, **ENERGY_TOL)
    np.testing.assert_allclose(np.array(rec.e2)[:, k], ref.e2, **ENERGY_TOL)


# ------------------------------------------------------------------ 1. the reference's captured iterates
@pytest.mark.parametrize("case", CASES)
def test_instance_zero_is_the_captured_reference_iterate(case):
    d, args, rec, x = _recorded(case, ("c",))
    assert rec.it == list(d["cp_it"])
    assert np.array_equal(np.array(rec.x)[:, 0], d["cp_x"])
    assert np.array_equal(x[0], d["cp_x"][-1])
    assert np.array_equal(np.array(rec.veq)[:, 0], np.asarray(d["cp_veq"], dtype=np.float64))
    assert np.array_equal(np.array(rec.vineq)[:, 0], d["cp_vineq"])
    np.testing.assert_allclose(np.array(rec.e1)[:, 0], d["cp_e1"], **ENERGY_TOL)
    np.testing.assert_allclose(np.array(rec.e2)[:, 0], d["cp_e2"], **ENERGY_TOL)


# ------------------------------------------------------------------ 2. the oracle, every instance
@pytest.mark.parametrize("case", CASES)
def test_every_instance_equals_the_oracle(case):
    d, args, rec, x = _recorded(case, ("c",))
    for k in range(B_BASE):
        _assert_instance_equals_oracle(d, args, rec, x, k)


@pytest.mark.parametrize("case", CASES)
def test_every_instance_equals_the_oracle_with_per_instance_rhs_bounds_and_start(case):
    d, args, rec, x = _recorded(case, ("c", "b", "bounds", "x0"))
    assert args["b_upper"].ndim == 2 and args["lb"].ndim == 2 and args["ub"].ndim == 2 and args["x0"].ndim == 2
    assert np.all(args["lb"] <= args["ub"])
    for k in range(B_BASE):
        _assert_instance_equals_oracle(d, args, rec, x, k)


@pytest.mark.parametrize("vary", [("c",), ("c", "b")])
def test_two_sided_rows_equal_the_oracle(vary):
    """b_lower finite on a third of the rows, b_upper infinite on a sixth: the stacking [A[up]; -A[lo]] (:74-88), shared and
    per instance."""
    d, args, rec, x = _recorded("random1", vary, True)
    lo, up = np.atleast_2d(args["b_lower"])[0] != -np.inf, np.atleast_2d(args["b_upper"])[0] != np.inf
    assert lo.any() and up.any() and (lo & up).any() and (lo & ~up).any() and (~lo & up).any()
    for k in range(B_BASE):
        _assert_instance_equals_oracle(d, args, rec, x, k)


# ------------------------------------------------------------------ 3. the shipped single-instance solver
def _states(args):
    """(batched state, [arguments of the single-instance CPState per instance]) for ``args``."""
    CPBatchState, _, CPState, _, one_sided_system, one_sided_system_batch, seq = _mods()
    a_ineq = args["a_ineq"]
    ineq, b_ineq = (None, None) if a_ineq is None else one_sided_system_batch(a_ineq, args["b_lower"], args["b_upper"])
    st = CPBatchState(args["c"], args["a_eq"], args["beq"], ineq, b_ineq, args["lb"], args["ub"], args["x0"], 1, 1)
    singles = []
    for k in range(args["c"].shape[0]):
        (c, a_eq, beq, _, bl, bu, lb, ub), x0 = _of_instance(args, k)
        ineq_k, b_k = (None, None) if a_ineq is None else one_sided_system(a_ineq, bl, bu)
        singles.append((c, a_eq, beq, ineq_k, b_k, lb, ub, x0, 1, 1, seq))
    return st, singles


def _single_result(single, iters):
    CPState = _mods()[2]
    st = CPState(*single)
    try:
        st.iterate(iters)
        st.primal_step()
        return st.x(), st.y(), st.report()[:5], st.preconditioners()
    finally:
        st.close()


@pytest.mark.parametrize("case", ["sc105", "potts50", "random2"])
def test_every_instance_equals_the_single_instance_solver(case):
    d = load_golden("lp_" + case)
    args = _instances(d, B_BASE, seed=3, vary=("c", "b", "bounds", "x0"))
    st, singles = _states(args)
    try:
        st.iterate(50)
        st.primal_step()
        x, y, rep = st.x(), st.y(), st.report()
        t, sigma = st.preconditioners()
    finally:
        st.close()
    for k, single in enumerate(singles):
        xs, ys, reps, (ts, ss) = _single_result(single, 50)
        assert np.array_equal(x[k], xs) and np.array_equal(y[k], ys)
        assert np.array_equal(rep[k, 2:], reps[2:])
        np.testing.assert_allclose(rep[k, :2], reps[:2], **ENERGY_TOL)
        assert np.array_equal(t, ts) and np.array_equal(sigma, ss)
    # and through the two public functions
    _, solve_batch, _, solve_one, _, _, seq = _mods()
    xb, _ = _run_batch(args, nb_max_iter=37, nb_iter_plot=10)
    for k in range(B_BASE):
        pos, x0 = _of_instance(args, k)
        x1, _ = solve_one(*pos, x0=x0, nb_max_iter=37, nb_iter_plot=10, order=seq, setup="host")
        assert np.array_equal(xb[k], x1)


# ------------------------------------------------------------------ 4. tile edges
TILE_ITERS = 25
TILE_BATCHES = [1, 2, 3, 8, 63, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def _tile_reference(case):
    """The 130 instances of the largest batch and the single-instance solver's result for each: every smaller batch is a prefix."""
    d = load_golden("lp_" + case)
    args = _instances(d, max(TILE_BATCHES), seed=41, vary=("c", "b", "bounds", "x0"))
    CPBatchState, _, _, _, one_sided_system, _, seq = _mods()
    ref = []
    for k in range(max(TILE_BATCHES)):
        (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = _of_instance(args, k)
        ineq_k, b_k = one_sided_system(a_ineq, bl, bu)
        ref.append(_single_result((c, a_eq, beq, ineq_k, b_k, lb, ub, x0, 1, 1, seq), TILE_ITERS)[:3])
    return args, ref


@pytest.mark.parametrize("batch", TILE_BATCHES)
@pytest.mark.parametrize("case", ["potts8", "random1"])
def test_tile_edges(case, batch):
    args, ref = _tile_reference(case)
    sub = {k: (v[:batch] if (k in ("c", "beq", "b_lower", "b_upper", "lb", "ub", "x0") and v is not None and np.ndim(v) == 2) else v)
           for k, v in args.items()}
    st, _ = _states(sub)
    try:
        assert st.batch == batch
        st.iterate(TILE_ITERS)
        st.primal_step()
        x, y, rep = st.x(), st.y(), st.report()
    finally:
        st.close()
    assert x.shape == (batch, args["c"].shape[1]) and rep.shape == (batch, 5)
    for k in range(batch):   # padding lanes never leak: every instance is the single-instance solver's, bit for bit
        xs, ys, reps = ref[k]
        assert np.array_equal(x[k], xs), k
        assert np.array_equal(y[k], ys), k
        assert np.array_equal(rep[k, 2:], reps[2:]), k
        np.testing.assert_allclose(rep[k, :2], reps[:2], **ENERGY_TOL)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("case", ["potts8", "sc50a"])
def test_instances_are_independent(case):
    d = load_golden("lp_" + case)
    args = _instances(d, 7, seed=9, vary=("c", "b", "bounds", "x0"))
    base, _ = _run_batch(args, nb_max_iter=40, nb_iter_plot=10)
    batched = ("c", "beq", "b_lower", "b_upper", "lb", "ub", "x0")

    def take(order):
        return {k: (v[order] if (k in batched and v is not None and np.ndim(v) == 2) else v) for k, v in args.items()}

    perm = np.random.RandomState(2).permutation(7)
    xp, _ = _run_batch(take(perm), nb_max_iter=40, nb_iter_plot=10)
    assert np.array_equal(xp, base[perm])
    dup = np.array([3, 0, 3, 5, 0, 3, 3, 1, 5])   # duplicated instances, a batch size of its own
    xd, _ = _run_batch(take(dup), nb_max_iter=40, nb_iter_plot=10)
    assert np.array_equal(xd, base[dup])
    assert np.array_equal(xd[0], xd[2]) and np.array_equal(xd[1], xd[4])


# ------------------------------------------------------------------ 6. cadence
def test_reporting_cadence_does_not_change_the_iterates():
    d = load_golden("lp_sc105")
    args = _instances(d, 6, seed=13, vary=("c", "x0"))
    finals, calls = [], []
    for plot in (1, 7, 10):
        rec = BatchRecorder()
        x, _ = _run_batch(args, nb_max_iter=45, nb_iter_plot=plot, callback_func=rec)
        finals.append(x)
        calls.append(rec.it)
    assert calls[0] == list(range(45)) and calls[1] == list(range(0, 45, 7)) and calls[2] == [0, 10, 20, 30, 40]
    assert np.array_equal(finals[0], finals[1]) and np.array_equal(finals[0], finals[2])
    # primal_step / report / dual_step against iterate
    a, _ = _states(args)
    b, _ = _states(args)
    try:
        a.iterate(12)
        for _ in range(12):
            b.primal_step()
            r = b.report()
            assert r.shape == (6, 5) and np.all(np.isfinite(r[:, :2]))
            b.dual_step()
        assert np.array_equal(a.x(), b.x()) and np.array_equal(a.y(), b.y())
    finally:
        a.close()
        b.close()


def test_max_time_zero_stops_the_whole_batch_at_the_first_report():
    d = load_golden("lp_random0")
    args = _instances(d, 4, seed=1, vary=("c",))
    rec = BatchRecorder()
    x, best = _run_batch(args, nb_max_iter=50, nb_iter_plot=10, max_time=0, callback_func=rec)
    assert rec.it == [] and best == [None] * 4
    st, _ = _states(args)
    try:
        st.primal_step()   # what the reference returns there: the primal half of iteration 0 is done (:198-228, :243)
        assert np.array_equal(x, st.x())
    finally:
        st.close()


# ------------------------------------------------------------------ 7. SparseLP.solve_batch
CURVES = ("pobj_curve", "dobj_curve", "max_violated_equality", "max_violated_inequality", "max_violated_constraint")


def _lp_case(name):
    from pysparselp_amd.SparseLP import SparseLP

    if name == "sc105_fixed":   # an LP with fixed variables: lb == ub on every ninth one
        lp = lp_from_golden(load_golden("lp_sc105"), SparseLP)
        fixed = np.arange(2, lp.nb_variables, 9)
        mid = np.where(np.isfinite(lp.upper_bounds[fixed]), 0.5 * (lp.lower_bounds[fixed] + lp.upper_bounds[fixed]), lp.lower_bounds[fixed] + 0.25)
        lp.lower_bounds[fixed] = mid
        lp.upper_bounds[fixed] = mid
        return lp
    return lp_from_golden(load_golden("lp_" + name), SparseLP)


@pytest.mark.parametrize("case", ["potts50", "sc105", "sc105_fixed"])
def test_solve_batch_equals_solve_per_instance(case):
    from pysparselp_amd import ORDER_SEQUENTIAL

    lp = _lp_case(case)
    if case.endswith("fixed"):
        assert np.any(lp.upper_bounds == lp.lower_bounds)
    batch, nb_iter = 4, 60
    rs = np.random.RandomState(23)
    costs = np.tile(lp.costsvector, (batch, 1))
    costs[1:] = lp.costsvector * (1 + 0.2 * rs.randn(batch - 1, lp.nb_variables)) + 0.05 * rs.randn(batch - 1, lp.nb_variables)
    x, elapsed = lp.solve_batch(costs, nb_iter=nb_iter, nb_iter_plot=10)
    assert x.shape == costs.shape and elapsed > 0
    assert lp.itrn_curve == [0, 10, 20, 30, 40, 50] and len(lp.opttime_curve) == 6 and len(lp.dopttime_curve) == 6
    for name in CURVES:
        assert all(np.shape(v) == (batch,) for v in getattr(lp, name)), name
    for k in range(batch):
        one = copy.deepcopy(lp)
        one.costsvector = costs[k].copy()
        xk = one.solve(method="chambolle_pock_ppd", get_timing=False, nb_iter=nb_iter, nb_iter_plot=10, setup="host", order=ORDER_SEQUENTIAL)
        assert np.array_equal(x[k], xk)
        assert one.itrn_curve == lp.itrn_curve
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.array(getattr(lp, name))[:, k], np.asarray(getattr(one, name), dtype=np.float64)), name
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(np.array(getattr(lp, name))[:, k], getattr(one, name), **ENERGY_TOL)
    assert lp.solve_batch(costs[:2], get_timing=False, nb_iter=5).shape == (2, lp.nb_variables)


# ------------------------------------------------------------------ 8. size
def test_potts256_batch16_against_the_oracle():
    from pysparselp_amd.problems import potts_lp

    lp = potts_lp(256)[0]
    n, batch = lp.nb_variables, 16
    rs = np.random.RandomState(4)
    cs = np.tile(lp.costsvector, (batch, 1))
    cs[1:, : 256 * 256] += 0.3 * rs.randn(batch - 1, 256 * 256)   # the unary costs
    solve = _mods()[1]
    a = (None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
    x, _ = solve(cs, *a, nb_max_iter=20, nb_iter_plot=20)
    assert x.shape == (batch, n)
    for k in (0, 7, 15):
        xo, _ = oracle.chambolle_pock_ppd(cs[k], *a, nb_max_iter=20, nb_iter_plot=20)
        assert np.array_equal(x[k], xo), k


# ------------------------------------------------------------------ 9. refusals
def _raw_create(lib, n, m_eq, m_ineq, indptr, indices, data, batch, b, c, lb, ub):
    from pysparselp_amd import _lib

    return lib.slp_cp_batch_create(n, m_eq, m_ineq, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data), batch, _lib.ptr(b), 0, _lib.ptr(c),
                                   _lib.ptr(lb), 0, _lib.ptr(ub), 0, None, 0, 1.0, 1.0)


def test_refusals_return_the_library_error_and_allocate_nothing():
    from pysparselp_amd import SlpError, _lib

    lib = _lib.lib()
    d = load_golden("lp_potts8")
    c, _, _, a_ineq, _, bu, lb, ub = _reduced(d)
    indptr, indices, data = _lib.csr_arrays(a_ineq)
    n, m = c.size, a_ineq.shape[0]
    c, lb, ub, bu = (_lib.f64(v) for v in (c, lb, ub, bu))
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.slp_device_memory(ctypes.byref(free), ctypes.byref(total)))
    # the first batch whose (5 n + 2 m) * 8 * B bytes of batched vectors alone exceed what is free (cached blocks included).  The
    # library checks before it reads a batched argument, so one row of costs stands for the B it would need.
    per_instance = (5 * n + 2 * m) * 8
    batch = (free.value + int(lib.slp_cached_bytes())) // per_instance + 1
    before = np.zeros(5)
    _lib.check(lib.slp_alloc_stats(_lib.ptr(before), 0))
    with pytest.raises(SlpError, match="device memory"):
        _lib.check_handle(_raw_create(lib, n, 0, m, indptr, indices, data, batch, bu, c, lb, ub))
    after = np.zeros(5)
    _lib.check(lib.slp_alloc_stats(_lib.ptr(after), 0))
    assert after[3] == before[3] and after[2] == before[2]   # no driver call, no byte more held
    # batch < 1
    for bad in (0, -3):
        with pytest.raises(SlpError, match="batch must be at least 1"):
            _lib.check_handle(_raw_create(lib, n, 0, m, indptr, indices, data, bad, bu, c, lb, ub))
    # a column index out of range is an error of the library too (the Python wrapper refuses it earlier)
    wrong = indices.copy()
    wrong[5] = n
    with pytest.raises(SlpError, match="column index out of range"):
        _lib.check_handle(_raw_create(lib, n, 0, m, indptr, wrong, data, 2, bu, np.tile(c, (2, 1)), lb, ub))
    # and the library still works
    h = _lib.check_handle(_raw_create(lib, n, 0, m, indptr, indices, data, 2, bu, np.tile(c, (2, 1)), lb, ub))
    lib.slp_cp_batch_destroy(h)
