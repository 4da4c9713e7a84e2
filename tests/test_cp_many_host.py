"""Host logic of Chambolle-Pock on a set of LPs (``chambolle_pock_ppd_many``, ``CPManyState``, ``SparseLP.solve_many``): every
refusal comes before the library is touched, and the block-diagonal assembly (offsets, row order, per-LP table) is the one the
device expects.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

from conftest import REPO, load_golden, lp_from_golden, solver_args
from pysparselp_amd import SparseLP as sparselp_module
from pysparselp_amd import _lib, chambolle_pock_ppd_many, solve_many
from pysparselp_amd.ChambollePockPPD import _many_problem, many_system, one_sided_system
from pysparselp_amd.SparseLP import SparseLP
from test_oracle_golden import CASES, _reduced


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load or bind the library fails the test: validation must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _problems(cases=("random1", "sc50a", "random0")):
    return [solver_args(load_golden("lp_" + c)) for c in cases]


def _with(problem, **changes):
    names = ("c", "a_eq", "beq", "a_ineq", "b_lower", "b_upper", "lb", "ub")
    return tuple(changes.get(name, v) for name, v in zip(names, problem))


def test_an_empty_list_is_refused(no_library):
    with pytest.raises(ValueError, match="empty list"):
        chambolle_pock_ppd_many([])
    with pytest.raises(ValueError, match="sequence of 8-tuples"):
        chambolle_pock_ppd_many(None)
    with pytest.raises(ValueError, match="empty list"):
        solve_many([])


def test_a_tuple_of_wrong_length_is_refused(no_library):
    ps = _problems()
    with pytest.raises(ValueError, match="LP 1 is not a tuple of 8"):
        chambolle_pock_ppd_many([ps[0], ps[1][:7], ps[2]])
    with pytest.raises(ValueError, match="LP 0 is not a tuple of 8"):
        chambolle_pock_ppd_many([ps[0] + (None,)])
    with pytest.raises(ValueError, match="LP 2 is not a tuple of 8"):
        chambolle_pock_ppd_many([ps[0], ps[1], 3.0])


def test_vectors_of_wrong_length_are_refused(no_library):
    ps = _problems()
    p = ps[1]   # sc50a: both kinds of rows
    assert p[1] is not None and p[3] is not None
    n, m_eq, m_in = p[0].size, p[1].shape[0], p[3].shape[0]
    bad = [
        ("c has shape", _with(p, c=np.zeros((2, n)))),
        ("c has shape", _with(p, c=np.zeros(0))),
        ("a_eq has .* columns", _with(p, c=p[0][:-1], lb=p[6][:-1], ub=p[7][:-1])),
        ("lb has shape", _with(p, lb=p[6][:-1])),
        ("ub has shape", _with(p, ub=np.zeros(n + 1))),
        ("beq has shape", _with(p, beq=np.zeros(m_eq + 1))),
        ("b_upper has shape", _with(p, b_upper=np.zeros(m_in - 1))),
        ("b_lower has shape", _with(p, b_lower=np.zeros(m_in + 2))),
    ]
    for match, problem in bad:
        with pytest.raises(ValueError, match="LP 1: " + match):
            chambolle_pock_ppd_many([ps[0], problem, ps[2]])
    wrong = scipy.sparse.csr_matrix(p[3])
    wrong.indices = wrong.indices.copy()
    wrong.indices[2] = n
    with pytest.raises(ValueError, match="LP 2: a_ineq has a column index outside"):
        chambolle_pock_ppd_many([ps[0], ps[2], _with(p, a_ineq=wrong)])


def test_x0_of_wrong_count_or_length_is_refused(no_library):
    ps = _problems()
    sizes = [p[0].size for p in ps]
    with pytest.raises(ValueError, match="sequence of 3 starts"):
        chambolle_pock_ppd_many(ps, x0=[np.zeros(sizes[0]), np.zeros(sizes[1])])
    with pytest.raises(ValueError, match="sequence of 3 starts"):
        chambolle_pock_ppd_many(ps, x0=0.0)
    with pytest.raises(ValueError, match="LP 1: x0 has shape"):
        chambolle_pock_ppd_many(ps, x0=[np.zeros(sizes[0]), np.zeros(sizes[1] + 1), None])


def test_an_accepted_call_gets_as_far_as_the_library(no_library):
    ps = _problems()
    with pytest.raises(AssertionError, match="library was loaded"):
        chambolle_pock_ppd_many(ps, x0=[None, np.zeros(ps[1][0].size), None], nb_max_iter=3)
    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("potts8", "random2")]
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_many(lps, nb_iter=3)


def test_lps_without_constraints_get_their_box_vertex(no_library):
    rng = np.random.RandomState(3)
    ps = []
    for n in (5, 1, 9):
        c = rng.randn(n)
        c[0] = 0.0
        ps.append((c, None, None, scipy.sparse.csr_matrix((0, n)), None, np.zeros(0), -rng.rand(n) - 1, rng.rand(n) + 1))
    xs, best = chambolle_pock_ppd_many(ps)
    assert best == [None] * 3
    for (c, *_, lb, ub), x in zip(ps, xs):
        assert np.array_equal(x, np.where(c > 0, lb, np.where(c < 0, ub, 0.0)))


def test_signatures():
    assert str(inspect.signature(chambolle_pock_ppd_many)) == (
        "(problems, x0=None, alpha=1, theta=1, nb_max_iter=100, callback_func=None, max_time=None, nb_iter_plot=10)")
    assert str(inspect.signature(solve_many)) == (
        "(lps, method='chambolle_pock_ppd', get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10)")
    assert sparselp_module.solve_many is solve_many


def test_solve_many_knows_one_method_and_the_pinned_tuples_stay(no_library):
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    for method in ("admm", "admm2", "dual_gradient_ascent", "nonsense"):
        with pytest.raises(ValueError, match="chambolle_pock_ppd"):
            solve_many(lps, method=method)
    assert sparselp_module.many_methods == ("chambolle_pock_ppd",)
    assert sparselp_module.solving_methods == ("chambolle_pock_ppd", "admm", "admm_blocks", "admm2")
    assert sparselp_module.dual_methods == ("dual_gradient_ascent",)
    assert sparselp_module.batch_methods == ("chambolle_pock_ppd",)


def _single_system(problem):
    """``K = [A_eq; K_ineq]`` and ``b`` of one LP as ``chambolle_pock_ppd`` stacks them on the host."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = problem
    blocks, b = [], []
    if a_eq is not None and a_eq.shape[0] > 0:
        blocks.append(scipy.sparse.csr_matrix(a_eq))
        b.append(np.asarray(beq, dtype=np.float64))
    if a_ineq is not None and a_ineq.shape[0] > 0:
        (p, j, v, rows), b_ineq = one_sided_system(a_ineq, bl, bu)
        blocks.append(scipy.sparse.csr_matrix((v, j, p), shape=(rows, c.size)))
        b.append(b_ineq)
    return blocks, b


@pytest.mark.parametrize("two_sided", [False, True])
def test_the_assembly_is_the_block_diagonal_of_the_single_systems(two_sided):
    problems = [_reduced(load_golden("lp_" + case)) for case in CASES]
    if two_sided:   # the one-sided stacking changes the row count of an LP (:74-88)
        problems.append(solver_args(load_golden("ka_l1svm")))
    assert any(p[1] is None or p[1].shape[0] == 0 for p in problems)   # LPs without equality rows are part of the set
    lps = [_many_problem(k, p) for k, p in enumerate(problems)]
    s = many_system(lps)
    count = len(problems)
    singles = [_single_system(p) for p in problems]
    n = np.array([p[0].size for p in problems])
    m_eq = np.array([0 if p[1] is None else p[1].shape[0] for p in problems])
    m_all = np.array([sum(blk.shape[0] for blk in blocks) for blocks, _ in singles])
    m_ineq = m_all - m_eq
    assert np.array_equal(s["n"], n) and np.array_equal(s["m_eq"], m_eq) and np.array_equal(s["m_ineq"], m_ineq)
    # the per-LP table: offsets of the columns and of the two row ranges
    assert np.array_equal(s["col0"], np.concatenate(([0], np.cumsum(n)[:-1])))
    assert np.array_equal(s["eq0"], np.concatenate(([0], np.cumsum(m_eq)[:-1])))
    assert np.array_equal(s["in0"], m_eq.sum() + np.concatenate(([0], np.cumsum(m_ineq)[:-1])))
    assert s["indptr"].dtype == np.int64 and s["indices"].dtype == np.int32 and s["data"].dtype == np.float64
    k_all = scipy.sparse.csr_matrix((s["data"], s["indices"], s["indptr"]), shape=(int(m_all.sum()), int(n.sum())))
    # against scipy's block diagonal of the per-LP K = [A_eq; A_ineq], its rows brought to "all equality rows, then all inequality rows"
    diag = scipy.sparse.block_diag([scipy.sparse.vstack(blocks) for blocks, _ in singles], format="csr")
    row0 = np.concatenate(([0], np.cumsum(m_all)[:-1]))
    order = np.concatenate([row0[k] + np.arange(m_eq[k]) for k in range(count)] + [row0[k] + m_eq[k] + np.arange(m_ineq[k]) for k in range(count)])
    want = diag[order]
    assert (k_all != want).nnz == 0 and k_all.nnz == sum(blk.nnz for blocks, _ in singles for blk in blocks)
    b_single = [np.concatenate(b) for _, b in singles]
    assert np.array_equal(s["b"], np.concatenate(b_single)[order])
    # every row keeps the entry order of its LP's own matrix (the sequential sums depend on it), columns offset by col0
    for k, (blocks, _) in enumerate(singles):
        own = scipy.sparse.vstack(blocks).tocsr() if len(blocks) > 1 else blocks[0]
        rows = np.concatenate((s["eq0"][k] + np.arange(m_eq[k]), s["in0"][k] + np.arange(m_ineq[k]))).astype(np.int64)
        for local in (0, len(rows) // 2, len(rows) - 1):
            g = rows[local]
            q0, q1 = s["indptr"][g], s["indptr"][g + 1]
            p0, p1 = own.indptr[local], own.indptr[local + 1]
            assert np.array_equal(s["indices"][q0:q1] - s["col0"][k], own.indices[p0:p1])
            assert np.array_equal(s["data"][q0:q1], own.data[p0:p1])
    for name, pos in (("c", 0), ("lb", 6), ("ub", 7)):
        assert np.array_equal(s[name], np.concatenate([p[pos] for p in problems]))


def _header_functions():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", text)))


def test_every_prototype_of_the_header_is_bound():
    names = ("create", "destroy", "iterate", "primal_step", "dual_step", "report", "get_x", "get_y", "get_preconditioners", "form",
             "lds_limit", "bench")
    declared = _header_functions()
    assert sorted(n for n in declared if n.startswith("slp_cp_many_")) == sorted("slp_cp_many_" + n for n in names)
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_cp_many_")) == sorted("slp_cp_many_" + n for n in names)
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared
    lib = _lib.load()   # dlopen works without a GPU
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.slp_cp_many_lds_limit() * 8 <= 160 * 1024


def test_the_layout_and_order_of_sums_give_the_reference_iterates():
    """The premise of the GPU parity tests, on the CPU: a restatement of what the device does with the assembled system -- stable
    transposition, T and Sigma over the whole, indices made local to their LP, a column walk and a row walk per LP in storage order
    with one accumulator -- reproduces the oracle's iterate of every LP bit for bit."""
    from oracle import oracle

    cases = ["sc50a", "potts8", "random0"]   # both kinds of rows; inequalities only with a finite b_lower; long rows
    problems = [_reduced(load_golden("lp_" + c)) for c in cases]
    s = many_system([_many_problem(k, p) for k, p in enumerate(problems)])
    n_all, m_eq_all = int(s["n"].sum()), int(s["m_eq"].sum())
    m_all = m_eq_all + int(s["m_ineq"].sum())
    ptr, idx, val = s["indptr"], s["indices"].astype(np.int64), s["data"]
    order = np.argsort(idx, kind="stable")   # build_transpose: rows increasing inside every column
    tidx, tval = np.repeat(np.arange(m_all), np.diff(ptr))[order], val[order]
    tptr = np.concatenate(([0], np.cumsum(np.bincount(idx, minlength=n_all))))
    t, sigma = np.empty(n_all), np.empty(m_all)
    for j in range(n_all):   # k_cp_colsum with the global m_eq (alpha = 1)
        se = si = 0.0
        for q in range(tptr[j], tptr[j + 1]):
            if tidx[q] < m_eq_all:
                se += abs(tval[q]) * 1.0
            else:
                si += abs(tval[q]) * 1.0
        tmp = (0.0 + se) + si
        t[j] = 1.0 / (tmp if tmp != 0 else 1.0)
    for i in range(m_all):   # k_cp_rowsum
        acc = 0.0
        for q in range(ptr[i], ptr[i + 1]):
            acc += abs(val[q]) * 1.0
        sigma[i] = 1.0 / (acc if acc != 0 else 1.0)

    def clip(v, lo, hi):
        v = v if (v > lo or v != v) else lo
        return v if (v < hi or v != v) else hi

    iters = 12
    for k, p in enumerate(problems):
        c0, n, me, mi, eq0, in0 = (int(s[name][k]) for name in ("col0", "n", "m_eq", "m_ineq", "eq0", "in0"))
        rows = [eq0 + r for r in range(me)] + [in0 + r for r in range(mi)]
        local = {g: r for r, g in enumerate(rows)}   # k_cpm_localise
        x, z, y = np.zeros(n), np.zeros(n), np.zeros(me + mi)
        for _ in range(iters):
            for j in range(n):
                se = si = 0.0
                for q in range(tptr[c0 + j], tptr[c0 + j + 1]):
                    r = local[tidx[q]]
                    if r < me:
                        se += tval[q] * y[r]
                    else:
                        si += tval[q] * y[r]
                cj = s["c"][c0 + j]
                d = (cj + se) + si if (me > 0 and mi > 0) else (cj + se if me > 0 else cj + si)
                x2 = clip(x[j] - t[c0 + j] * d, s["lb"][c0 + j], s["ub"][c0 + j])
                z[j] = 2.0 * x2 - 1.0 * x[j]
                x[j] = x2
            for r, g in enumerate(rows):
                kz = 0.0
                for q in range(ptr[g], ptr[g + 1]):
                    kz += val[q] * z[idx[q] - c0]
                yn = y[r] + sigma[g] * (kz - s["b"][g])
                y[r] = 0.0 if (r >= me and yn < 0.0) else yn
        want, _ = oracle.chambolle_pock_ppd(*p, nb_max_iter=iters, nb_iter_plot=1000)
        assert np.array_equal(x, want), cases[k]
