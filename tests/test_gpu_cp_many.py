"""Chambolle-Pock on a set of LPs with different matrices, one workgroup per LP (csrc/slp_cp_many.hip, ``chambolle_pock_ppd_many``,
``CPManyState``, ``SparseLP.solve_many``) on the GPU.

Every LP of a set must be BIT FOR BIT the iterate of the reference (golden fixtures) and of the shipped single solver in
SEQUENTIAL order -- ``x``, ``y`` and the three maxima of the report with ``np.array_equal``; the report's two energies are sums in
another fixed order: ``rtol = atol = 1e-9``, the bar of ``test_gpu_cp_batch`` and ``test_gpu_admm_batch`` for such sums.

The single-solver references are computed once per LP and shared (never modified).  Needs a real MI355X: run with ``-m gpu``.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse

from conftest import Recorder, lp_from_golden, load_golden, solver_args
from test_gpu_parity import CASES
from test_oracle_golden import _reduced

pytestmark = pytest.mark.gpu

ENERGY_TOL = dict(rtol=1e-9, atol=1e-9)
STOPS = (1, 2, 11, 51)
FORMS = (None, "lds", "global")


def _mods():
    from pysparselp_amd import ORDER_SEQUENTIAL, CPManyState, chambolle_pock_ppd_many
    from pysparselp_amd.ChambollePockPPD import CPState, _many_problem, chambolle_pock_ppd, many_lds_limit, one_sided_system

    return CPManyState, chambolle_pock_ppd_many, CPState, chambolle_pock_ppd, one_sided_system, _many_problem, many_lds_limit, ORDER_SEQUENTIAL


@pytest.fixture()
def form_env(monkeypatch):
    """Sets the two switches the library reads when a set is created."""
    def use(form=None, kmax=None):
        for name, v in (("SLP_CP_MANY_FORM", form), ("SLP_CP_MANY_KMAX", kmax)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))

    use()
    yield use
    use()


def _advance(state, k, pieces):
    """``k`` whole iterations in uneven ``iterate`` calls."""
    for p in pieces:
        p = min(p, k)
        state.iterate(p)
        k -= p
    state.iterate(k)


def _walk(state, stops, get):
    """The state at every stop: ``stop - 1`` iterations further in uneven calls, then a reporting iteration (primal half, report,
    dual half).  Returns ``[(x, y, report)]``."""
    out, done = [], 0
    for s in stops:
        _advance(state, s - 1 - done, (3, 1, 7))
        state.primal_step()
        rep = state.report()
        state.dual_step()
        done = s
        out.append(get(state) + (np.array(rep, copy=True),))
    return out


def _single_walk(problem, x0=None, stops=STOPS):
    """The single solver in SEQUENTIAL order on one LP: ``[(x, y, report[:5])]`` at the stops."""
    CPState, one_sided_system, order = _mods()[2], _mods()[4], _mods()[7]
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    if a_eq is not None and a_eq.shape[0] == 0:
        a_eq, beq = None, None
    ineq, b_ineq = (None, None) if (a_ineq is None or a_ineq.shape[0] == 0) else one_sided_system(a_ineq, bl, bu)
    st = CPState(c, a_eq, beq, ineq, b_ineq, lb, ub, x0, 1, 1, order)
    try:
        return [(x, y, rep[:5]) for x, y, rep in _walk(st, stops, lambda s: (s.x(), s.y()))]
    finally:
        st.close()


def _many_walk(problems, x0=None, stops=STOPS):
    """The set solver: per stop ``(xs, ys, report (count, 5))``, and the form of every LP."""
    CPManyState, prep = _mods()[0], _mods()[5]
    st = CPManyState([prep(k, p) for k, p in enumerate(problems)], x0)
    try:
        forms = [st.form(k) for k in range(st.count)]
        return _walk(st, stops, lambda s: (s.x(), s.y())), forms
    finally:
        st.close()


def _assert_lp_equal(got, k, want):
    """LP ``k`` of a set walk against a single walk, at every stop."""
    assert len(got) == len(want)
    for (xs, ys, rep), (x, y, r) in zip(got, want):
        assert np.array_equal(xs[k], x)
        assert np.array_equal(ys[k], y)
        assert np.array_equal(rep[k, 2:5], r[2:5]), (rep[k], r)
        np.testing.assert_allclose(rep[k, :2], r[:2], **ENERGY_TOL)


@functools.lru_cache(maxsize=None)
def _fixture_problem(case):
    return _reduced(load_golden("lp_" + case))


@functools.lru_cache(maxsize=None)
def _fixture_single(case):
    return _single_walk(_fixture_problem(case))


# ------------------------------------------------------------------ 1. the reference's captured iterates
class ManyRecorder:
    """Collects the callback calls of the set solver (copies)."""

    def __init__(self):
        self.it, self.x, self.e1, self.e2, self.veq, self.vineq = [], [], [], [], [], []

    def __call__(self, niter, xs, e1, e2, dur, veq, vineq):
        self.it.append(niter)
        self.x.append([np.array(x, copy=True) for x in xs])
        for store, v in ((self.e1, e1), (self.e2, e2), (self.veq, veq), (self.vineq, vineq)):
            store.append(np.array(v, dtype=np.float64, copy=True))


def test_every_fixture_in_one_call_is_the_captured_reference_iterate(form_env):
    CPManyState, solve_many_cp, prep = _mods()[0], _mods()[1], _mods()[5]
    golden = [load_golden("lp_" + case) for case in CASES]
    problems = [_fixture_problem(case) for case in CASES]
    limit = _mods()[6]()
    # the automatic choice mixes the forms: potts50 exceeds any budget inside 160 KiB, the others fit
    st = CPManyState([prep(k, p) for k, p in enumerate(problems)])
    try:
        forms = [st.form(k) for k in range(st.count)]
    finally:
        st.close()
    assert limit * 8 <= 160 * 1024
    for case, p, f in zip(CASES, problems, forms):
        size = 2 * p[0].size + p[1].shape[0] + p[3].shape[0]
        assert f == ("lds" if size <= limit else "global"), case
    assert forms[CASES.index("potts50")] == "global" and forms.count("lds") == len(CASES) - 1
    last = max(int(d["cp_it"][-1]) for d in golden)
    rec = ManyRecorder()
    xs, _ = solve_many_cp(problems, nb_max_iter=last + 1, callback_func=rec, nb_iter_plot=1)
    assert rec.it == list(range(last + 1))
    for k, d in enumerate(golden):
        its = [int(i) for i in d["cp_it"]]
        assert np.array_equal(np.array([rec.x[i][k] for i in its]), d["cp_x"]), CASES[k]
        assert np.array_equal(np.array([rec.veq[i][k] for i in its]), np.asarray(d["cp_veq"], dtype=np.float64)), CASES[k]
        assert np.array_equal(np.array([rec.vineq[i][k] for i in its]), d["cp_vineq"]), CASES[k]
        np.testing.assert_allclose([rec.e1[i][k] for i in its], d["cp_e1"], **ENERGY_TOL)
        np.testing.assert_allclose([rec.e2[i][k] for i in its], d["cp_e2"], **ENERGY_TOL)
        if its[-1] == last:
            assert np.array_equal(xs[k], d["cp_x"][-1])


# ------------------------------------------------------------------ 2. against the single solver
@pytest.mark.parametrize("form, kmax", [(None, None), ("lds", None), ("global", None), (None, 1), ("lds", 1)])
def test_every_lp_equals_the_single_solver_at_every_stop(form_env, form, kmax):
    cases = [c for c in CASES if not (form == "lds" and c == "potts50")]
    form_env(form, kmax)
    got, forms = _many_walk([_fixture_problem(c) for c in cases])
    if form is not None:
        assert set(forms) == {form}
    for k, c in enumerate(cases):
        _assert_lp_equal(got, k, _fixture_single(c))


# ------------------------------------------------------------------ 3. independence and offsets
@pytest.mark.parametrize("form", FORMS)
def test_a_permuted_list_gives_the_permuted_results(form_env, form):
    cases = ["random1", "sc105", "potts8", "random0", "sc50a", "random2"]
    perm = [4, 0, 5, 2, 1, 3]
    form_env(form)
    stops = (1, 12)
    base, _ = _many_walk([_fixture_problem(c) for c in cases], stops=stops)
    moved, _ = _many_walk([_fixture_problem(cases[i]) for i in perm], stops=stops)
    for (xs, ys, rep), (xm, ym, repm) in zip(base, moved):
        for to, frm in enumerate(perm):
            assert np.array_equal(xm[to], xs[frm]) and np.array_equal(ym[to], ys[frm])
            assert np.array_equal(repm[to], rep[frm])   # the report's order of sums is a function of the LP's shape only


@pytest.mark.parametrize("form", FORMS)
def test_an_lp_alone_equals_the_same_lp_among_the_others(form_env, form):
    form_env(form)
    cases = ["sc50a", "random2", "sc105"]
    among, _ = _many_walk([_fixture_problem(c) for c in cases])
    for k, c in enumerate(cases):
        alone, forms = _many_walk([_fixture_problem(c)])   # count = 1
        assert len(forms) == 1
        for (xs, ys, rep), (xa, ya, repa) in zip(among, alone):
            assert np.array_equal(xs[k], xa[0]) and np.array_equal(ys[k], ya[0]) and np.array_equal(rep[k], repa[0])
        _assert_lp_equal(alone, 0, _fixture_single(c))


def test_count_one_in_the_global_form_with_a_start(form_env):
    p = _fixture_problem("potts50")
    x0 = 0.1 * np.random.RandomState(8).randn(p[0].size)
    got, forms = _many_walk([p], x0=[x0], stops=(1, 6))
    assert forms == ["global"]
    _assert_lp_equal(got, 0, _single_walk(p, x0=x0, stops=(1, 6)))


def test_more_lps_than_compute_units(form_env):
    """300 perturbed copies of SC50A (matrix values and costs), each checked against the single solver."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = _fixture_problem("sc50a")
    rs = np.random.RandomState(300)
    problems = []
    for k in range(300):
        ae, ai = scipy.sparse.csr_matrix(a_eq), scipy.sparse.csr_matrix(a_ineq)
        ae.data = ae.data * (1 + 0.1 * rs.randn(ae.nnz))
        ai.data = ai.data * (1 + 0.1 * rs.randn(ai.nnz))
        problems.append((c * (1 + 0.2 * rs.randn(c.size)) + 0.05 * rs.randn(c.size), ae, beq, ai, bl, bu, lb, ub))
    stops = (21,)
    got, forms = _many_walk(problems, stops=stops)
    assert forms == ["lds"] * 300
    for k, p in enumerate(problems):
        _assert_lp_equal(got, k, _single_walk(p, stops=stops))


# ------------------------------------------------------------------ 4. edges
def _random_lp(rs, n, m_eq, m_in, lengths=(3,), empty_rows=(), lower=False):
    """A seeded LP with rows of the given entry counts (cycled), columns in no particular order inside a row."""
    def block(m, first):
        ptr, idx = [0], []
        for r in range(m):
            k = 0 if (first + r) in empty_rows else min(n, lengths[(first + r) % len(lengths)])
            idx.extend(rs.choice(n, size=k, replace=False))
            ptr.append(len(idx))
        a = scipy.sparse.csr_matrix((rs.randn(len(idx)), np.array(idx, dtype=np.int32), np.array(ptr)), shape=(m, n))
        return a if m > 0 else None

    a_eq, a_in = block(m_eq, 0), block(m_in, m_eq)
    c = rs.randn(n)
    lb, ub = -rs.rand(n) - 0.5, rs.rand(n) + 0.5
    beq = 0.1 * rs.randn(m_eq) if m_eq else None
    bu = rs.rand(m_in)
    bl = None
    if lower and m_in:   # rows with both bounds, a lower bound only, an upper bound only
        bl = np.full(m_in, -np.inf)
        bl[0::3] = bu[0::3] - 1.5
        bu[0::6] = np.inf
    return c, a_eq, beq, a_in, bl, bu, lb, ub


@functools.lru_cache(maxsize=None)
def _edge_set():
    limit = _mods()[6]()
    rs = np.random.RandomState(41)
    named = [
        ("one_variable", _random_lp(rs, 1, 1, 2, lengths=(1,))),
        ("one_row", _random_lp(rs, 7, 0, 1, lengths=(4,))),
        # rows 1 and 5 without entries; the rows touch few of the 40 columns, so there are empty columns too
        ("empty_rows_and_columns", _random_lp(rs, 40, 3, 6, lengths=(2, 1), empty_rows=(1, 5))),
        ("equalities_only", _random_lp(rs, 30, 12, 0, lengths=(3, 5))),
        ("inequalities_only", _random_lp(rs, 33, 0, 20, lengths=(4, 2), lower=True)),
        # more columns than the widest workgroup has lanes (1024): lanes loop; rows of 1, 4, 5 and 9 entries (the four-ahead tail)
        ("wide", _random_lp(rs, 2500, 35, 70, lengths=(1, 4, 5, 9))),
        ("narrow", _random_lp(rs, 11, 4, 9, lengths=(1, 4, 5, 9))),
        # 2 n + m exactly the LDS budget, and one double more
        ("at_the_limit", _random_lp(rs, (limit - 2000) // 2, 500, limit - 2 * ((limit - 2000) // 2) - 500, lengths=(3, 1, 6))),
        ("past_the_limit", _random_lp(rs, (limit - 2000) // 2, 500, limit + 1 - 2 * ((limit - 2000) // 2) - 500, lengths=(3, 1, 6))),
    ]
    empty = named[2][1]
    stacked = scipy.sparse.vstack([empty[1], empty[3]]).tocsc()
    assert np.any(np.diff(stacked.indptr) == 0) and np.any(np.diff(empty[1].indptr) == 0) and np.any(np.diff(empty[3].indptr) == 0)
    return named


@functools.lru_cache(maxsize=None)
def _edge_single(name):
    return _single_walk(dict(_edge_set())[name], stops=(1, 2, 13))


@pytest.mark.parametrize("form", FORMS)
def test_edge_shapes_equal_the_single_solver(form_env, form):
    limit = _mods()[6]()
    named = [(name, p) for name, p in _edge_set() if not (form == "lds" and name == "past_the_limit")]
    form_env(form)
    got, forms = _many_walk([p for _, p in named], stops=(1, 2, 13))
    sizes = {name: 2 * p[0].size + (0 if p[1] is None else p[1].shape[0]) + (0 if p[3] is None else p[3].shape[0]) for name, p in named}
    assert sizes["at_the_limit"] == limit
    if form is None:
        assert sizes["past_the_limit"] == limit + 1
        assert forms == ["lds"] * (len(named) - 1) + ["global"]   # the budget decides, one double past it included
    else:
        assert set(forms) == {form}
    for k, (name, _) in enumerate(named):
        _assert_lp_equal(got, k, _edge_single(name))


# ------------------------------------------------------------------ 5. finite b_lower
def test_lps_with_finite_b_lower_equal_their_single_solves(form_env):
    solve_many_cp, solve_one, order = _mods()[1], _mods()[3], _mods()[7]
    problems = [solver_args(load_golden("ka_l1svm")), solver_args(load_golden("lp_sc105")), solver_args(load_golden("ka_kmedians"))]
    for p in (problems[0], problems[2]):
        assert p[4] is not None and np.max(p[4]) > -np.inf
    rec = ManyRecorder()
    xs, best = solve_many_cp(problems, nb_max_iter=25, nb_iter_plot=10, callback_func=rec)
    assert rec.it == [0, 10, 20] and len(xs) == 3 and len(best) == 3
    for k, p in enumerate(problems):
        one = Recorder()
        x, _ = solve_one(*p, nb_max_iter=25, nb_iter_plot=10, order=order, setup="host", callback_func=one)
        assert np.array_equal(xs[k], x), k
        assert one.it == rec.it
        for i in range(3):
            assert np.array_equal(rec.x[i][k], one.x[i])
            assert rec.veq[i][k] == one.veq[i] and rec.vineq[i][k] == one.vineq[i]
            np.testing.assert_allclose([rec.e1[i][k], rec.e2[i][k]], [one.e1[i], one.e2[i]], **ENERGY_TOL)


# ------------------------------------------------------------------ 6. SparseLP.solve_many
def _solve_many_lps():
    from pysparselp_amd.SparseLP import SparseLP

    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("sc50a", "potts8", "random1", "sc105")]
    lp = lps[2]   # a tenth of its variables fixed through equal bounds
    fixed = np.arange(0, lp.nb_variables, 10)
    value = np.clip(0.25, lp.lower_bounds[fixed], lp.upper_bounds[fixed])
    lp.lower_bounds[fixed] = value
    lp.upper_bounds[fixed] = value
    return lps


def test_solve_many_equals_solve_per_lp(form_env):
    from pysparselp_amd import ORDER_SEQUENTIAL, solve_many

    lps, singles = _solve_many_lps(), _solve_many_lps()
    xs, elapsed = solve_many(lps, nb_iter=60, nb_iter_plot=10)
    assert elapsed > 0 and len(xs) == 4
    assert np.array_equal(solve_many(_solve_many_lps(), get_timing=False, nb_iter=60, nb_iter_plot=10)[2], xs[2])
    for k, lp in enumerate(singles):
        x, _ = lp.solve(method="chambolle_pock_ppd", nb_iter=60, nb_iter_plot=10, order=ORDER_SEQUENTIAL, setup="host")
        assert x.shape == (lp.nb_variables,) and np.array_equal(xs[k], x), k
        got = lps[k]
        assert got.itrn_curve == lp.itrn_curve == [0, 10, 20, 30, 40, 50]
        for name in ("max_violated_equality", "max_violated_inequality", "max_violated_constraint"):
            assert np.array_equal(np.asarray(getattr(got, name), dtype=np.float64), np.asarray(getattr(lp, name), dtype=np.float64)), (k, name)
        for name in ("pobj_curve", "dobj_curve"):
            np.testing.assert_allclose(getattr(got, name), getattr(lp, name), **ENERGY_TOL)
        assert len(got.opttime_curve) == len(got.dopttime_curve) == 6


def test_solve_many_max_time_zero_stops_at_the_first_report(form_env):
    from pysparselp_amd import solve_many

    lps = _solve_many_lps()
    xs = solve_many(lps, get_timing=False, nb_iter=60, nb_iter_plot=10, max_time=0)
    for lp, x in zip(lps, xs):
        assert lp.itrn_curve == [] and lp.pobj_curve == [] and x.shape == (lp.nb_variables,)


# ------------------------------------------------------------------ 7. refusals of the C ABI
def _device_free(lib):
    from pysparselp_amd import _lib

    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.slp_device_memory(ctypes.byref(free), ctypes.byref(total)))
    return free.value


def test_refusals_return_the_library_error_and_allocate_nothing(form_env):
    from pysparselp_amd import SlpError, _lib
    from pysparselp_amd.ChambollePockPPD import many_system

    lib, prep = _lib.lib(), _mods()[5]

    def system(cases):
        return many_system([prep(k, _fixture_problem(c)) for k, c in enumerate(cases)])

    def create(s, count=None, indices=None):
        return lib.slp_cp_many_create(len(s["n"]) if count is None else count, _lib.ptr(s["n"]), _lib.ptr(s["m_eq"]), _lib.ptr(s["m_ineq"]),
                                      _lib.ptr(s["indptr"]), _lib.ptr(s["indices"] if indices is None else indices), _lib.ptr(s["data"]),
                                      _lib.ptr(s["b"]), _lib.ptr(s["c"]), _lib.ptr(s["lb"]), _lib.ptr(s["ub"]), None, 1.0, 1.0)

    def refused(match, *a, **k):
        before, stats0 = _device_free(lib), np.zeros(5)
        _lib.check(lib.slp_alloc_stats(_lib.ptr(stats0), 0))
        with pytest.raises(SlpError, match=match):
            _lib.check_handle(create(*a, **k))
        stats1 = np.zeros(5)
        _lib.check(lib.slp_alloc_stats(_lib.ptr(stats1), 0))
        assert _device_free(lib) == before
        assert stats1[3] == stats0[3] and stats1[2] == stats0[2]   # no driver call, no byte more held

    s = system(["sc50a", "random0"])
    for bad in (0, -2):
        refused("count must be at least 1", s, count=bad)
    # an index of LP 1 that points into LP 0's columns: inside the concatenated matrix, outside its LP
    wrong = s["indices"].copy()
    row = int(s["eq0"][1])
    wrong[s["indptr"][row]] = 3
    refused("outside the LP's columns", s, indices=wrong)
    wrong = s["indices"].copy()
    wrong[-1] = int(s["n"].sum())
    refused("outside the LP's columns", s, indices=wrong)
    backwards = dict(s, indptr=s["indptr"].copy())
    backwards["indptr"][2] = backwards["indptr"][1] - 1
    refused("non-decreasing", backwards)
    form_env("lds")
    refused("SLP_CP_MANY_FORM=lds, but LP 1 needs", system(["sc50a", "potts50"]))
    form_env("neither")
    refused("must be lds or global", s)
    form_env()
    h = _lib.check_handle(create(s))   # the same arguments, untouched, are accepted
    lib.slp_cp_many_destroy(h)


def test_the_launch_cap_switch_is_parsed_strictly(form_env):
    """A value that is not a positive number -- trailing text included -- is refused before anything is allocated."""
    from pysparselp_amd import SlpError

    CPManyState, prep = _mods()[0], _mods()[5]
    lps = [prep(k, _fixture_problem(c)) for k, c in enumerate(("random0", "random1"))]
    for bad in ("0", "abc", "7x"):
        form_env(kmax=bad)
        with pytest.raises(SlpError, match="SLP_CP_MANY_KMAX must be a positive number of iterations"):
            CPManyState(lps)
