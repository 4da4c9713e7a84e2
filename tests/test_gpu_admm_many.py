"""ADMM with the projected Gauss-Seidel x-step on a list of LPs (csrc/slp_admm_many.hip, ``lp_admm_many``, ``ADMMManyState``,
``solve_admm_many``) on the GPU.

Every LP of a list must be BIT FOR BIT the iterate of the reference (golden fixtures) and of the shipped single solver in
SEQUENTIAL order on that LP alone: ``x``, ``lambda``, ``max |A x - b|`` and ``max(0, -min x)`` are compared with
``np.array_equal``.  The energy is a sum in a fixed order of its own: ``rtol = atol = 1e-9``, the bar of
``test_gpu_admm_batch.py`` for a fixed-order sum in another order.  Single-solver references are computed once per LP and
cached.  Needs a real MI355X: run with ``-m gpu``.
"""
import functools

import numpy as np
import pytest

from conftest import lp_from_golden, load_golden, solver_args
from test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

ENERGY_TOL = dict(rtol=1e-9, atol=1e-9)
SMALL = [c for c in CASES if c != "potts50"]
STOPS = (1, 2, 11, 51)        # sweeps done when the states are compared
ADVANCE = (3, 1, 7)           # uneven iterate() calls between two stops; the rest in one


def _mods():
    from pysparselp_amd import ORDER_SEQUENTIAL, ADMMManyState, lp_admm_many
    from pysparselp_amd.ADMM import ADMMBatchState, ADMMState, _admm_many_problem, _admm_many_starts

    return ADMMManyState, lp_admm_many, ADMMState, ADMMBatchState, ORDER_SEQUENTIAL, _admm_many_problem, _admm_many_starts


@functools.lru_cache(maxsize=None)
def _problem(case):
    return solver_args(load_golden("lp_" + case))


def _many_state(problems, x0=None, **kw):
    ADMMManyState, _, _, _, _, prep, starts = _mods()
    lps = [prep(k, p) for k, p in enumerate(problems)]
    return ADMMManyState(lps, starts(x0, lps), **kw)


def _advance(st, k):
    for step in ADVANCE:
        if k >= step:
            st.iterate(step)
            k -= step
    st.iterate(k)


def _walk(st, snap):
    """The state at every stop of STOPS: after ``stop - 1`` iterations and the sweep of the next one."""
    out, done = [], 0
    for stop in STOPS:
        _advance(st, stop - 1 - done)
        st.sweep_step()
        out.append(snap(st))
        st.multiplier_step()
        done = stop
    return out


def _single_walk(problem, x0=None, gamma_eq=2, gamma_ineq=3, use_preconditioning=True):
    ADMMState, seq = _mods()[2], _mods()[4]
    st = ADMMState.from_lp(*problem, x0, gamma_eq, gamma_ineq, use_preconditioning, order=seq)
    try:
        return _walk(st, lambda s: (s.x(), s.lam(), s.report()[:3].copy()))
    finally:
        st.close()


@functools.lru_cache(maxsize=None)
def _single_reference(case):
    """(x over all N, lambda, report) of the single solver in SEQUENTIAL order at every stop (never modified)."""
    return _single_walk(_problem(case))


def _many_walk(problems, x0=None, **kw):
    st = _many_state(problems, x0, **kw)
    try:
        return _walk(st, lambda s: (s.x(full=True), s.lam(), s.report()))
    finally:
        st.close()


def _same(got, k, want):
    """Stop by stop: LP ``k`` of the list's walk against a single walk."""
    for (xs, lams, rep), (x, lam, r) in zip(got, want):
        assert np.array_equal(xs[k], x) and np.array_equal(lams[k], lam), k
        assert np.array_equal(rep[k, 1:], r[1:]), k
        np.testing.assert_allclose(rep[k, 0], r[0], **ENERGY_TOL)


class ListRecorder:
    def __init__(self, keep):
        self.keep = set(int(k) for k in keep)
        self.it, self.x, self.e1, self.veq, self.vineq = [], [], [], [], []

    def __call__(self, niter, sols, e1, e2, dur, veq, vineq):
        if niter in self.keep:
            self.it.append(niter)
            self.x.append([np.array(v, copy=True) for v in sols])
            for store, v in ((self.e1, e1), (self.veq, veq), (self.vineq, vineq)):
                store.append(np.array(v, dtype=np.float64, copy=True))


# ------------------------------------------------------------------ 1. the reference's captured iterates
def test_every_lp_is_the_captured_reference_iterate():
    golden = [load_golden("lp_" + c) for c in CASES]
    last = max(int(d["admm_it"][-1]) for d in golden)
    rec = ListRecorder(np.concatenate([d["admm_it"] for d in golden]))
    xs = _mods()[1]([_problem(c) for c in CASES], nb_iter=last, callback_func=rec, nb_iter_plot=1)
    assert len(xs) == len(CASES)
    for k, d in enumerate(golden):
        at = [rec.it.index(int(i)) for i in d["admm_it"]]
        assert np.array_equal(np.array([rec.x[t][k] for t in at]), d["admm_x"]), CASES[k]
        assert np.array_equal(np.array([rec.veq[t][k] for t in at]), np.asarray(d["admm_veq"], dtype=np.float64)), CASES[k]
        assert np.array_equal(np.array([rec.vineq[t][k] for t in at]), np.asarray(d["admm_vineq"], dtype=np.float64)), CASES[k]
        np.testing.assert_allclose(np.array([rec.e1[t][k] for t in at]), d["admm_e1"], **ENERGY_TOL)


# ------------------------------------------------------------------ 2. the shipped single solver, LP by LP
@functools.lru_cache(maxsize=None)
def _list_walk():
    return _many_walk([_problem(c) for c in CASES])


def test_every_lp_equals_the_single_solver():
    got = _list_walk()
    for k, case in enumerate(CASES):
        _same(got, k, _single_reference(case))


# ------------------------------------------------------------------ 3. forms, launch cap
def test_forms_by_shape():
    from pysparselp_amd.ADMM import admm_many_lds_limit

    assert admm_many_lds_limit() * 8 == 160000
    st = _many_state([_problem(c) for c in CASES])
    try:
        for k, case in enumerate(CASES):
            p = _problem(case)
            doubles = 2 * (p[0].size + p[3].shape[0]) + (0 if p[1] is None else p[1].shape[0]) + p[3].shape[0]
            assert (doubles == 44200) if case == "potts50" else (doubles <= 1024)
            assert st.form(k) == ("global" if case == "potts50" else "lds"), case
        assert 1 <= st.kmax("lds") <= 1024 and 1 <= st.kmax("global") <= 1024
        with pytest.raises(IndexError):
            st.form(len(CASES))
    finally:
        st.close()


def test_the_global_form_gives_the_same_iterates(monkeypatch):
    monkeypatch.setenv("SLP_ADMM_MANY_FORM", "global")
    st = _many_state([_problem(c) for c in CASES])
    try:
        assert all(st.form(k) == "global" for k in range(len(CASES))) and st.kmax("lds") == 0
        got = _walk(st, lambda s: (s.x(full=True), s.lam(), s.report()))
    finally:
        st.close()
    for k, case in enumerate(CASES):
        _same(got, k, _single_reference(case))


def test_the_lds_form_refuses_an_lp_that_does_not_fit(monkeypatch):
    from pysparselp_amd import SlpError

    monkeypatch.setenv("SLP_ADMM_MANY_FORM", "lds")
    with pytest.raises(SlpError, match="LP 1 needs 44200 doubles"):
        _many_state([_problem("sc50a"), _problem("potts50"), _problem("random0")])
    got = _many_walk([_problem(c) for c in SMALL])
    for k, case in enumerate(SMALL):
        _same(got, k, _single_reference(case))
    monkeypatch.setenv("SLP_ADMM_MANY_FORM", "nonsense")
    with pytest.raises(SlpError, match="SLP_ADMM_MANY_FORM"):
        _many_state([_problem("sc50a")])


def test_one_iteration_per_launch_gives_the_same_iterates(monkeypatch):
    monkeypatch.setenv("SLP_ADMM_MANY_KMAX", "1")
    st = _many_state([_problem(c) for c in CASES])
    try:
        assert st.kmax("lds") == 1 and st.kmax("global") == 1
        got = _walk(st, lambda s: (s.x(full=True), s.lam(), s.report()))
    finally:
        st.close()
    for k, case in enumerate(CASES):
        _same(got, k, _single_reference(case))


# ------------------------------------------------------------------ 4. levels
def test_every_lp_has_the_levels_of_its_own_plan():
    """Potts-50's widest level (4901 rows) is wider than the workgroup; SC50A's levels are a few rows wide.  The composite of
    the list has more than 4096 sink rows, each LP but Potts-50 far fewer: the plan's rule on them is applied per LP."""
    ADMMBatchState = _mods()[3]
    st = _many_state([_problem(c) for c in CASES])
    try:
        for k, case in enumerate(CASES):
            p = _problem(case)
            one = ADMMBatchState(p[0][None, :], *p[1:])
            try:
                assert st.num_levels(k) == one.num_levels() > 1, case
            finally:
                one.close()
    finally:
        st.close()


# ------------------------------------------------------------------ 5. independence
def test_permuting_the_list_permutes_the_results():
    perm = np.random.RandomState(5).permutation(len(CASES))
    got = _many_walk([_problem(CASES[j]) for j in perm])
    for k, j in enumerate(perm):
        _same(got, k, _single_reference(CASES[j]))


def test_a_list_longer_than_the_compute_units():
    order = [SMALL[k % len(SMALL)] for k in range(260)]
    got = _many_walk([_problem(c) for c in order])
    assert len(got[0][0]) == 260 and got[0][2].shape == (260, 3)
    for k, case in enumerate(order):
        _same(got, k, _single_reference(case))


@pytest.mark.parametrize("case", ["sc50a", "potts50"])
def test_a_list_of_one_lp(case):
    _same(_many_walk([_problem(case)]), 0, _single_reference(case))


# ------------------------------------------------------------------ 6. warm starts
def test_warm_starts_with_none_entries():
    cases = ["sc105", "potts8", "random1", "sc50a"]
    rs = np.random.RandomState(11)
    x0 = [0.3 * rs.randn(_problem(cases[0])[0].size), None, rs.rand(_problem(cases[2])[0].size) - 0.5, None]
    got = _many_walk([_problem(c) for c in cases], x0)
    for k, case in enumerate(cases):
        _same(got, k, _single_reference(case) if x0[k] is None else _single_walk(_problem(case), x0[k]))
    assert not np.array_equal(got[0][0][0], _single_reference(cases[0])[0][0])


# ------------------------------------------------------------------ 7. shared parameters
@pytest.mark.parametrize("kw", [dict(use_preconditioning=False), dict(gamma_eq=1.5, gamma_ineq=0.7)], ids=["unscaled", "gammas"])
def test_shared_parameters(kw):
    cases = ["random2", "sc50a", "potts8"]
    got = _many_walk([_problem(c) for c in cases], **kw)
    for k, case in enumerate(cases):
        _same(got, k, _single_walk(_problem(case), **kw))


# ------------------------------------------------------------------ 8. solve_admm_many
CURVES = ("pobj_curve", "dobj_curve", "max_violated_equality", "max_violated_inequality", "max_violated_constraint")


def test_solve_admm_many_equals_solve_per_lp():
    from pysparselp_amd import ORDER_SEQUENTIAL, solve_admm_many
    from pysparselp_amd.SparseLP import SparseLP

    cases = ["sc105", "potts8", "random0"]
    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in cases]
    nb_iter = 40
    xs, elapsed = solve_admm_many(lps, nb_iter=nb_iter, nb_iter_plot=10)
    assert len(xs) == 3 and elapsed > 0
    for k, case in enumerate(cases):
        lp = lps[k]
        one = lp_from_golden(load_golden("lp_" + case), SparseLP)
        xk = one.solve(method="admm", get_timing=False, nb_iter=nb_iter, nb_iter_plot=10, setup="host", order=ORDER_SEQUENTIAL)
        assert np.array_equal(xs[k], xk), case
        assert lp.itrn_curve == one.itrn_curve == [0, 10, 20, 30, 40] and len(lp.opttime_curve) == 5 and len(lp.dopttime_curve) == 5
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.asarray(getattr(lp, name), dtype=np.float64), np.asarray(getattr(one, name), dtype=np.float64)), name
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(getattr(lp, name), getattr(one, name), **ENERGY_TOL)
    assert len(solve_admm_many(lps[:2], get_timing=False, nb_iter=5)) == 2


def test_the_launch_cap_switch_is_parsed_strictly(monkeypatch):
    """A value that is not a positive number -- trailing text included -- is refused before anything is allocated."""
    from pysparselp_amd import SlpError

    for bad in ("0", "abc", "7x"):
        monkeypatch.setenv("SLP_ADMM_MANY_KMAX", bad)
        with pytest.raises(SlpError, match="SLP_ADMM_MANY_KMAX must be a positive number of iterations"):
            _many_state([_problem("random0"), _problem("random1")])
