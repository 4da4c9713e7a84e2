"""Batched ADMM with the projected Gauss-Seidel x-step (csrc/slp_admm_batch.hip, ``lp_admm_batch``,
``SparseLP.solve_admm_batch``) on the GPU.

Every instance of a batch must be BIT FOR BIT the iterate of the reference (golden fixtures, the oracle) and of the shipped
single-instance solver in SEQUENTIAL order: ``x``, ``lambda``, ``max |A x - b|`` and ``max(0, -min x)`` are compared with
``np.array_equal``.  The energy is a sum in a fixed order of its own: ``rtol = atol = 1e-9``, the bar of the batched
Chambolle-Pock tests for their fixed-order sums.  Every case runs in BOTH forms of the iteration (``SLP_ADMM_BATCH_FORM``).

Instances are built from the golden fixtures with seeded ``numpy.random.RandomState`` draws; instance 0 is always the fixture
itself and instance 1 has exact zeros among its costs.  Lanes of padding instances are idle in every kernel and their state
cannot be read through the C ABI; what a test can see of them is that a batch which needs padding gives the same instances
as one that does not (tile edges, independence).  Needs a real MI355X: run with ``-m gpu``.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse

from conftest import Recorder, lp_from_golden, load_golden, solver_args
from oracle import oracle
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

ENERGY_TOL = dict(rtol=1e-9, atol=1e-9)
FORMS = ["tile", "levels"]


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    monkeypatch.setenv("SLP_ADMM_BATCH_FORM", request.param)
    return request.param


def _mods():
    from pysparselp_amd import ORDER_SEQUENTIAL, ADMMBatchState, lp_admm_batch
    from pysparselp_amd.ADMM import ADMMState

    return ADMMBatchState, lp_admm_batch, ADMMState, ORDER_SEQUENTIAL


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


def _instances(d, batch, seed, vary=("c",)):
    """The fixture's LP as ``batch`` instances: a dict of the arguments of ``lp_admm_batch``.  ``vary`` names what differs between
    the instances (the others stay shared vectors); instance 0 is the fixture unperturbed."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = solver_args(d)
    rs = np.random.RandomState(seed)
    n = c.size
    cs = np.tile(c, (batch, 1))
    cs[1:] = c * (1 + 0.2 * rs.randn(batch - 1, n)) + 0.05 * np.mean(np.abs(c)) * rs.randn(batch - 1, n)
    if batch > 1:
        cs[1, ::3] = 0.0
    args = dict(cs=cs, a_eq=a_eq, beq=beq, a_ineq=a_ineq, b_lower=bl, b_upper=bu, lb=lb, ub=ub, x0=None)
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


BATCHED = ("cs", "lb", "ub", "x0")


def _take(args, order):
    return {k: (v[order] if (k in BATCHED and v is not None and np.ndim(v) == 2) else v) for k, v in args.items()}


def _of_instance(args, k):
    """The positional arguments (and x0) of a single-instance solver for instance ``k``."""
    pick = lambda v: v if (v is None or np.ndim(v) == 1) else v[k]  # noqa: E731
    return ((args["cs"][k], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], pick(args["lb"]),
             pick(args["ub"])), pick(args["x0"]))


def _run_batch(args, **kw):
    return _mods()[1](args["cs"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"], args["ub"],
                      x0=args["x0"], **kw)


def _state(args):
    return _mods()[0](args["cs"], args["a_eq"], args["beq"], args["a_ineq"], args["b_lower"], args["b_upper"], args["lb"], args["ub"],
                      args["x0"])


def _state_result(args, iters):
    """(x over all N, lambda) after ``iters`` iterations and the sweep of the next one."""
    st = _state(args)
    try:
        st.iterate(iters)
        st.sweep_step()
        return st.x(), st.lam(), st.report()
    finally:
        st.close()


# ------------------------------------------------------------------ 1. the reference's captured iterates
@pytest.mark.parametrize("case", CASES)
def test_instance_zero_is_the_captured_reference_iterate(case, form):
    d = load_golden("lp_" + case)
    args = _instances(d, 3, seed=len(case))
    rec = BatchRecorder(d["admm_it"])
    x = _run_batch(args, nb_iter=int(d["admm_it"][-1]), callback_func=rec, nb_iter_plot=1)
    assert rec.it == list(d["admm_it"])
    assert np.array_equal(np.array(rec.x)[:, 0], d["admm_x"])
    assert np.array_equal(x[0], d["admm_x"][-1])
    assert np.array_equal(np.array(rec.veq)[:, 0], np.asarray(d["admm_veq"], dtype=np.float64))
    assert np.array_equal(np.array(rec.vineq)[:, 0], np.asarray(d["admm_vineq"], dtype=np.float64))
    np.testing.assert_allclose(np.array(rec.e1)[:, 0], d["admm_e1"], **ENERGY_TOL)


# ------------------------------------------------------------------ 2. the oracle, every instance
ORACLE_ITERS = 40
ORACLE_BATCH = 4


@functools.lru_cache(maxsize=None)
def _oracle_reference(case, vary):
    """Instances of the fixture and, per instance, the oracle's callbacks of every iteration, its final x, and its full iterate
    and multipliers after the last sweep (never modified; shared by both forms)."""
    d = load_golden("lp_" + case)
    args = _instances(d, ORACLE_BATCH, seed=len(case) + 17 * len(vary), vary=vary)
    refs = []
    for k in range(ORACLE_BATCH):
        pos, x0 = _of_instance(args, k)
        rec, last = Recorder(), {}

        def hook(i, xn, x, lam, last=last):
            if i == ORACLE_ITERS:
                last["x"], last["lam"] = x.copy(), lam.copy()

        xo = oracle.lp_admm(*pos, x0=x0, nb_iter=ORACLE_ITERS, callback_func=rec, nb_iter_plot=1, iterate_hook=hook)
        refs.append((rec, xo, last))
    return args, refs


@pytest.mark.parametrize("vary", [("c",), ("c", "bounds", "x0")], ids=["costs", "costs_bounds_start"])
@pytest.mark.parametrize("case", ["sc105", "potts8", "potts50", "random1"])
def test_every_instance_equals_the_oracle(case, vary, form):
    args, refs = _oracle_reference(case, vary)
    if "bounds" in vary:
        assert args["lb"].ndim == 2 and args["ub"].ndim == 2 and args["x0"].ndim == 2 and np.all(args["lb"] <= args["ub"])
    assert np.any(args["cs"][1] == 0.0)
    rec = BatchRecorder()
    x = _run_batch(args, nb_iter=ORACLE_ITERS, callback_func=rec, nb_iter_plot=1)
    xs, lams, _ = _state_result(args, ORACLE_ITERS)
    for k, (ref, xo, last) in enumerate(refs):
        assert rec.it == ref.it
        assert np.array_equal(np.array(rec.x)[:, k], np.array(ref.x)), k
        assert np.array_equal(x[k], xo), k
        assert np.array_equal(np.array(rec.veq)[:, k], np.asarray(ref.veq, dtype=np.float64)), k
        assert np.array_equal(np.array(rec.vineq)[:, k], np.asarray(ref.vineq, dtype=np.float64)), k
        np.testing.assert_allclose(np.array(rec.e1)[:, k], ref.e1, **ENERGY_TOL)
        assert np.array_equal(xs[k], last["x"]) and np.array_equal(lams[k], last["lam"]), k


# ------------------------------------------------------------------ 3. the shipped single-instance solver
@pytest.mark.parametrize("case", ["sc105", "potts50", "random2"])
def test_every_instance_equals_the_single_instance_solver(case, form):
    _, _, ADMMState, seq = _mods()
    d = load_golden("lp_" + case)
    args = _instances(d, 5, seed=3, vary=("c", "bounds", "x0"))
    x, lam, rep = _state_result(args, 30)
    for k in range(5):
        (c, a_eq, beq, a_ineq, bl, bu, lb, ub), x0 = _of_instance(args, k)
        st = ADMMState.from_lp(c, a_eq, beq, a_ineq, bl, bu, lb, ub, x0, 2, 3, True, order=seq)
        try:
            st.iterate(30)
            st.sweep_step()
            assert np.array_equal(x[k], st.x()) and np.array_equal(lam[k], st.lam()), k
            r = st.report()[:3]
            assert np.array_equal(rep[k, 1:], r[1:])
            np.testing.assert_allclose(rep[k, 0], r[0], **ENERGY_TOL)
        finally:
            st.close()


# ------------------------------------------------------------------ 4. tile edges
# The shipped rule chooses tile widths 1, 4 and 16: every B one below, at and one above them, one B over three tiles of the
# widest (40), and the sizes at which the tile form's rule changes the width (256 | 257, 1024 | 1025).
TILE_ITERS = 12
TILE_DISTINCT = 17
TILE_BATCHES = [1, 2, 3, 4, 5, 15, 16, 17, 40]
TILE_RULE_BATCHES = [255, 256, 257, 1023, 1024, 1025]


@functools.lru_cache(maxsize=None)
def _tile_reference(case, form):
    """17 distinct instances and each of them solved in a batch of 1 (in the form under test); larger batches repeat them."""
    d = load_golden("lp_" + case)
    args = _instances(d, TILE_DISTINCT, seed=41, vary=("c", "bounds", "x0"))
    return args, [_state_result(_take(args, np.array([k])), TILE_ITERS) for k in range(TILE_DISTINCT)]


def _check_tile_edge(case, batch, form):
    args, ref = _tile_reference(case, form)
    order = np.arange(batch) % TILE_DISTINCT
    x, lam, rep = _state_result(_take(args, order), TILE_ITERS)
    assert x.shape[0] == batch and lam.shape[0] == batch and rep.shape == (batch, 3)
    for k in range(batch):
        xs, ls, rs = ref[order[k]]
        assert np.array_equal(x[k], xs[0]) and np.array_equal(lam[k], ls[0]), k
        assert np.array_equal(rep[k, 1:], rs[0, 1:]), k
        np.testing.assert_allclose(rep[k, 0], rs[0, 0], **ENERGY_TOL)


@pytest.mark.parametrize("batch", TILE_BATCHES)
@pytest.mark.parametrize("case", ["potts8", "random1"])
def test_tile_edges(case, batch, form):
    _check_tile_edge(case, batch, form)


@pytest.mark.parametrize("batch", TILE_RULE_BATCHES)
def test_tile_edges_where_the_rule_changes_the_width(batch, form):
    _check_tile_edge("potts8", batch, form)


def test_form_switch_and_default_rule(monkeypatch):
    d = load_golden("lp_potts8")
    args = _instances(d, 3, seed=1)
    for want in FORMS:
        monkeypatch.setenv("SLP_ADMM_BATCH_FORM", want)
        st = _state(args)
        try:
            assert st.form() == want and st.num_levels() > 1
        finally:
            st.close()
    monkeypatch.delenv("SLP_ADMM_BATCH_FORM")
    st = _state(args)
    try:
        assert st.form() == "tile"   # narrow levels
    finally:
        st.close()
    from pysparselp_amd import SlpError

    monkeypatch.setenv("SLP_ADMM_BATCH_FORM", "nonsense")
    with pytest.raises(SlpError, match="SLP_ADMM_BATCH_FORM"):
        _state(args)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("case", ["potts8", "sc50a"])
def test_instances_are_independent(case, form):
    d = load_golden("lp_" + case)
    args = _instances(d, 7, seed=9, vary=("c", "bounds", "x0"))
    x, lam, _ = _state_result(args, 25)
    changed = copy.deepcopy(args)
    changed["cs"][3] = changed["cs"][3] * 1.5 + 0.25
    x2, lam2, _ = _state_result(changed, 25)
    others = np.array([0, 1, 2, 4, 5, 6])
    assert np.array_equal(x2[others], x[others]) and np.array_equal(lam2[others], lam[others])
    assert not np.array_equal(x2[3], x[3])
    perm = np.random.RandomState(2).permutation(7)
    xp, lamp, _ = _state_result(_take(args, perm), 25)
    assert np.array_equal(xp, x[perm]) and np.array_equal(lamp, lam[perm])
    # a batch that needs padding (5 of a tile of 16 in the levels form) and prefixes of it give the same instances
    x5, lam5, _ = _state_result(_take(args, np.arange(5)), 25)
    assert np.array_equal(x5, x[:5]) and np.array_equal(lam5, lam[:5])


# ------------------------------------------------------------------ 6. k iterations in one launch
@pytest.mark.parametrize("k", [7, 70])   # 70 is above the most iterations one launch of the tile form holds (64)
def test_k_iterations_in_one_call_equal_k_calls_of_one(k, form):
    d = load_golden("lp_sc105")
    args = _instances(d, 6, seed=13, vary=("c", "x0"))
    a, b, c = _state(args), _state(args), _state(args)
    try:
        a.iterate(k)
        for _ in range(k):
            b.iterate(1)
            c.sweep_step()
            c.multiplier_step()
        xa, la = a.x(), a.lam()
        assert np.array_equal(xa, b.x()) and np.array_equal(la, b.lam())
        assert np.array_equal(xa, c.x()) and np.array_equal(la, c.lam())
    finally:
        a.close()
        b.close()
        c.close()


# ------------------------------------------------------------------ 7. cadence, max_time
def test_reporting_cadence_does_not_change_the_iterates(form):
    d = load_golden("lp_sc105")
    args = _instances(d, 6, seed=13, vary=("c", "x0"))
    finals, calls = [], []
    for plot in (1, 3, 10):
        rec = BatchRecorder()
        finals.append(_run_batch(args, nb_iter=45, nb_iter_plot=plot, callback_func=rec))
        calls.append(rec.it)
    assert calls[0] == list(range(46)) and calls[1] == list(range(0, 46, 3)) and calls[2] == [0, 10, 20, 30, 40]
    assert np.array_equal(finals[0], finals[1]) and np.array_equal(finals[0], finals[2])


def test_max_time_zero_stops_the_whole_batch_at_the_first_report(form):
    d = load_golden("lp_random0")
    args = _instances(d, 4, seed=1)
    rec = BatchRecorder()
    x = _run_batch(args, nb_iter=50, nb_iter_plot=10, max_time=0, callback_func=rec)
    assert rec.it == []
    st = _state(args)
    try:
        st.sweep_step()   # what the reference returns there: the sweep of iteration 0 is done (:162, :213-216)
        assert np.array_equal(x, st.x(x.shape[1]))
    finally:
        st.close()


# ------------------------------------------------------------------ 8. absent equality block, a single dependency level
def _against_oracle(args, iters, form):
    rec = BatchRecorder()
    x = _run_batch(args, nb_iter=iters, callback_func=rec, nb_iter_plot=1)
    for k in range(args["cs"].shape[0]):
        pos, x0 = _of_instance(args, k)
        ref = Recorder()
        xo = oracle.lp_admm(*pos, x0=x0, nb_iter=iters, callback_func=ref, nb_iter_plot=1)
        assert np.array_equal(x[k], xo), k
        assert np.array_equal(np.array(rec.x)[:, k], np.array(ref.x)), k
        assert np.array_equal(np.array(rec.veq)[:, k], np.asarray(ref.veq, dtype=np.float64)), k
        assert np.array_equal(np.array(rec.vineq)[:, k], np.asarray(ref.vineq, dtype=np.float64)), k
        np.testing.assert_allclose(np.array(rec.e1)[:, k], ref.e1, **ENERGY_TOL)


def test_no_equality_block_matches_the_oracle(form):
    args = _instances(load_golden("lp_random1"), 4, seed=5, vary=("c", "x0"))
    assert args["a_eq"] is not None
    args["a_eq"], args["beq"] = None, None
    _against_oracle(args, 30, form)


def test_single_dependency_level_matches_the_oracle(form):
    """Equality rows with one entry each on distinct columns and inequality rows without stored entries: no two unknowns of the
    standard form share a row, M is diagonal, the sweep has one level."""
    rs = np.random.RandomState(8)
    n = 9
    a_eq = scipy.sparse.csr_matrix((rs.rand(4) + 0.5, (np.arange(4), [1, 3, 4, 7])), shape=(4, n))
    args = dict(cs=rs.randn(5, n), a_eq=a_eq, beq=rs.rand(4), a_ineq=scipy.sparse.csr_matrix((2, n)), b_lower=None,
                b_upper=np.array([1.0, 2.0]), lb=np.zeros(n), ub=np.ones(n), x0=0.3 * rs.rand(5, n))
    st = _state(args)
    try:
        assert st.num_levels() == 1
    finally:
        st.close()
    _against_oracle(args, 20, form)


# ------------------------------------------------------------------ 9. SparseLP.solve_admm_batch
CURVES = ("pobj_curve", "dobj_curve", "max_violated_equality", "max_violated_inequality", "max_violated_constraint")


@pytest.mark.parametrize("case", ["potts50", "sc105"])
def test_solve_admm_batch_equals_solve_per_instance(case, form):
    from pysparselp_amd import ORDER_SEQUENTIAL
    from pysparselp_amd.SparseLP import SparseLP

    lp = lp_from_golden(load_golden("lp_" + case), SparseLP)
    batch, nb_iter = 3, 40
    rs = np.random.RandomState(23)
    costs = np.tile(lp.costsvector, (batch, 1))
    costs[1:] = lp.costsvector * (1 + 0.2 * rs.randn(batch - 1, lp.nb_variables)) + 0.05 * rs.randn(batch - 1, lp.nb_variables)
    x, elapsed = lp.solve_admm_batch(costs, nb_iter=nb_iter, nb_iter_plot=10)
    assert x.shape == costs.shape and elapsed > 0
    assert lp.itrn_curve == [0, 10, 20, 30, 40] and len(lp.opttime_curve) == 5 and len(lp.dopttime_curve) == 5
    for name in CURVES:
        assert all(np.shape(v) == (batch,) for v in getattr(lp, name)), name
    for k in range(batch):
        one = copy.deepcopy(lp)
        one.costsvector = costs[k].copy()
        xk = one.solve(method="admm", get_timing=False, nb_iter=nb_iter, nb_iter_plot=10, setup="host", order=ORDER_SEQUENTIAL)
        assert np.array_equal(x[k], xk)
        assert one.itrn_curve == lp.itrn_curve
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.array(getattr(lp, name))[:, k], np.asarray(getattr(one, name), dtype=np.float64)), name
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(np.array(getattr(lp, name))[:, k], getattr(one, name), **ENERGY_TOL)
    assert lp.solve_admm_batch(costs[:2], get_timing=False, nb_iter=5).shape == (2, lp.nb_variables)


# ------------------------------------------------------------------ 10. size
@functools.lru_cache(maxsize=None)
def _potts256():
    from pysparselp_amd.problems import potts_lp

    lp = potts_lp(256)[0]
    batch = 3
    rs = np.random.RandomState(4)
    cs = np.tile(lp.costsvector, (batch, 1))
    cs[1:, : 256 * 256] += 0.3 * rs.randn(batch - 1, 256 * 256)   # the unary costs
    a = (None, None, lp.a_inequalities, lp.b_lower, lp.b_upper, lp.lower_bounds, lp.upper_bounds)
    return cs, a, [oracle.lp_admm(cs[k], *a, nb_iter=1, nb_iter_plot=100) for k in range(batch)]


def test_potts256_batch3_against_the_oracle(form):
    """The full-size Potts LP of tests/test_gpu_potts256.py (256 x 256 grid, N = 457 216 unknowns in standard form, 512 levels),
    B = 3, two iterations; the three oracle solves take under a second together on the CPU."""
    cs, a, refs = _potts256()
    x = _mods()[1](cs, *a, nb_iter=1, nb_iter_plot=100)
    assert x.shape == cs.shape
    for k, xo in enumerate(refs):
        assert np.array_equal(x[k], xo), k


# ------------------------------------------------------------------ 11. refusals
def _raw_create(lib, n, eq, beq, m_ineq, ineq, bu, batch, c, lb, ub):
    from pysparselp_amd import _lib

    m_eq = 0 if eq is None else eq[0].size - 1
    eq_ptrs = (None, None, None) if eq is None else tuple(_lib.ptr(v) for v in eq)
    in_ptrs = (None, None, None) if ineq is None else tuple(_lib.ptr(v) for v in ineq)
    return lib.slp_admm_batch_create_lp(n, m_eq, *eq_ptrs, _lib.ptr(beq), m_ineq, *in_ptrs, None, _lib.ptr(bu), batch, _lib.ptr(c), 1,
                                        _lib.ptr(lb), 0, _lib.ptr(ub), 0, None, 0, 2.0, 3.0, 1)


def _device_free(lib):
    from pysparselp_amd import _lib

    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.slp_device_memory(ctypes.byref(free), ctypes.byref(total)))
    return free.value


def test_refusals_return_the_library_error_and_allocate_nothing():
    from pysparselp_amd import SlpError, _lib

    lib = _lib.lib()
    d = load_golden("lp_sc105")
    c, a_eq, beq, a_ineq, _, bu, lb, ub = solver_args(d)
    eq, ineq = _lib.csr_arrays(a_eq), _lib.csr_arrays(a_ineq)
    n, m_eq, m_ineq = c.size, a_eq.shape[0], a_ineq.shape[0]
    c, lb, ub, bu, beq = (_lib.f64(v) for v in (c, lb, ub, bu, beq))
    two = np.tile(c, (2, 1))

    def refused(match, *a):
        before, stats0 = _device_free(lib), np.zeros(5)
        _lib.check(lib.slp_alloc_stats(_lib.ptr(stats0), 0))
        with pytest.raises(SlpError, match=match):
            _lib.check_handle(_raw_create(lib, *a))
        stats1 = np.zeros(5)
        _lib.check(lib.slp_alloc_stats(_lib.ptr(stats1), 0))
        assert _device_free(lib) == before
        assert stats1[3] == stats0[3] and stats1[2] == stats0[2]   # no driver call, no byte more held

    for bad in (0, -3):
        refused("batch must be at least 1", n, eq, beq, m_ineq, ineq, bu, bad, two, lb, ub)
    refused("inequality block is required", n, eq, beq, 0, None, bu, 2, two, lb, ub)
    wrong = (ineq[0], ineq[1].copy(), ineq[2])
    wrong[1][5] = n
    refused("column index out of range", n, eq, beq, m_ineq, wrong, bu, 2, two, lb, ub)
    wrong_eq = (eq[0], eq[1].copy(), eq[2])
    wrong_eq[1][0] = -1
    refused("column index out of range", n, wrong_eq, beq, m_ineq, ineq, bu, 2, two, lb, ub)
    # the first batch whose (3 N + m + n) * 8 * B bytes of batched vectors alone exceed what is free (cached blocks included).
    # The library checks before it reads a batched argument, so two rows of costs stand for the B it would need.
    per_instance = (3 * (n + m_ineq) + (m_eq + m_ineq) + n) * 8
    batch = (_device_free(lib) + int(lib.slp_cached_bytes())) // per_instance + 1
    refused("device memory", n, eq, beq, m_ineq, ineq, bu, batch, two, lb, ub)
    # and the library still works
    h = _lib.check_handle(_raw_create(lib, n, eq, beq, m_ineq, ineq, bu, 2, two, lb, ub))
    lib.slp_admm_batch_destroy(h)
