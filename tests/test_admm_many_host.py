"""Host logic of ADMM on a list of LPs (``lp_admm_many``, ``ADMMManyState``, ``admm_many_system``, ``solve_admm_many``): every
refusal comes before the library is touched and names the LP, the block-diagonal assembly (offsets, row order, per-LP table) is
the one the device expects, and the premise of the GPU parity tests holds on the CPU -- the set-up chain and the iterations of
``lp_admm`` on the composite give every LP the bits of its own solve.  None of it needs a GPU."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse

import pysparselp_amd
from conftest import REPO, load_golden, lp_from_golden, solver_args
from pysparselp_amd import SparseLP as sparselp_module
from pysparselp_amd import _lib, lp_admm_many, solve_admm_many, solve_many
from pysparselp_amd.ADMM import _admm_many_problem, admm_many_system
from pysparselp_amd.SparseLP import SparseLP


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


def _poisoned(v, at, value):
    out = np.array(v, dtype=np.float64, copy=True)
    out[at] = value
    return out


# ------------------------------------------------------------------ refusals
def test_an_empty_list_is_refused(no_library):
    with pytest.raises(ValueError, match="empty list"):
        lp_admm_many([])
    with pytest.raises(ValueError, match="sequence of 8-tuples"):
        lp_admm_many(None)
    with pytest.raises(ValueError, match="empty list"):
        solve_admm_many([])


def test_an_entry_that_is_no_8_tuple_is_refused(no_library):
    ps = _problems()
    with pytest.raises(ValueError, match="LP 1 is not a tuple of 8"):
        lp_admm_many([ps[0], ps[1][:7], ps[2]])
    with pytest.raises(ValueError, match="LP 0 is not a tuple of 8"):
        lp_admm_many([ps[0] + (None,)])
    with pytest.raises(ValueError, match="LP 2 is not a tuple of 8"):
        lp_admm_many([ps[0], ps[1], 3.0])


def test_an_lp_without_an_inequality_block_is_refused(no_library):
    ps = _problems()
    with pytest.raises(ValueError, match="LP 1 has no inequality block.*tools.py:92"):
        lp_admm_many([ps[0], _with(ps[1], a_ineq=None, b_lower=None, b_upper=None), ps[2]])
    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("potts8", "sc50a")]
    lps[1].a_inequalities = scipy.sparse.csr_matrix((0, lps[1].nb_variables))
    with pytest.raises(ValueError, match="LP 1 has no inequality block"):
        solve_admm_many(lps, nb_iter=3)


def test_shape_mismatches_are_refused(no_library):
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
        ("a_eq without beq", _with(p, beq=None)),
        ("b_upper has shape", _with(p, b_upper=np.zeros(m_in - 1))),
        ("b_lower has shape", _with(p, b_lower=np.zeros(m_in + 2))),
    ]
    for match, problem in bad:
        with pytest.raises(ValueError, match="LP 1: " + match):
            lp_admm_many([ps[0], problem, ps[2]])
    narrow = scipy.sparse.csr_matrix(p[3])[:, : n - 1]
    with pytest.raises(ValueError, match="LP 0: a_ineq has .* columns"):
        lp_admm_many([_with(p, a_ineq=narrow)])


def test_a_column_index_out_of_range_is_refused(no_library):
    ps = _problems()
    p = ps[1]
    for name, pos, at, value in (("a_ineq", 3, 2, p[0].size), ("a_eq", 1, 0, -1)):
        wrong = scipy.sparse.csr_matrix(p[pos])
        wrong.indices = wrong.indices.copy()
        wrong.indices[at] = value
        with pytest.raises(ValueError, match=f"LP 2: {name} has a column index outside"):
            lp_admm_many([ps[0], ps[2], _with(p, **{name: wrong})])


def test_a_nan_in_a_right_hand_side_or_bound_is_refused(no_library):
    ps = _problems()
    p = ps[1]
    for name, pos in (("beq", 2), ("b_upper", 5), ("lb", 6), ("ub", 7)):
        with pytest.raises(ValueError, match=f"LP 1: {name} has a NaN"):
            lp_admm_many([ps[0], _with(p, **{name: _poisoned(p[pos], 1, np.nan)}), ps[2]])
    two_sided = ps[0]
    assert two_sided[4] is not None
    with pytest.raises(ValueError, match="LP 0: b_lower has a NaN"):
        lp_admm_many([_with(two_sided, b_lower=_poisoned(two_sided[4], 0, np.nan))])
    # infinite sides and bounds are the reference's way to say "none": accepted as far as the library
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_admm_many([_with(two_sided, b_lower=_poisoned(two_sided[4], 0, -np.inf), ub=_poisoned(two_sided[7], 0, np.inf))])


def test_a_cost_or_start_that_is_not_finite_is_refused(no_library):
    ps = _problems()
    for value in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="LP 2: c has an entry that is not finite"):
            lp_admm_many([ps[0], ps[1], _with(ps[2], c=_poisoned(ps[2][0], 3, value))])
        with pytest.raises(ValueError, match="LP 1: x0 has an entry that is not finite"):
            lp_admm_many(ps, x0=[None, _poisoned(np.zeros(ps[1][0].size), 0, value), None])
    sizes = [p[0].size for p in ps]
    with pytest.raises(ValueError, match="sequence of 3 starts"):
        lp_admm_many(ps, x0=[np.zeros(sizes[0]), np.zeros(sizes[1])])
    with pytest.raises(ValueError, match="sequence of 3 starts"):
        lp_admm_many(ps, x0=0.0)
    with pytest.raises(ValueError, match="LP 1: x0 has shape"):
        lp_admm_many(ps, x0=[np.zeros(sizes[0]), np.zeros(sizes[1] + 1), None])


def test_a_list_of_2_to_the_31_unknowns_or_rows_is_refused(no_library):
    """The sizes alone decide: stand-ins with the shapes of huge LPs (nothing of that size is allocated)."""
    def stub(n, m_eq, m_in):
        block = lambda rows: types.SimpleNamespace(shape=(rows, n))  # noqa: E731
        return (types.SimpleNamespace(size=n), block(m_eq) if m_eq else None, None, block(m_in), None, None, None, None)

    for lps in ([stub(2 ** 30, 0, 2 ** 29), stub(2 ** 29, 0, 1)],        # variables + slacks
                [stub(5, 2 ** 30, 2 ** 29), stub(7, 2 ** 29, 3)]):        # rows
        with pytest.raises(ValueError, match=r"2\^31 or more variables \+ slacks or rows"):
            admm_many_system(lps)


def test_an_accepted_call_gets_as_far_as_the_library(no_library):
    ps = _problems()
    with pytest.raises(AssertionError, match="library was loaded"):
        lp_admm_many(ps, x0=[None, np.zeros(ps[1][0].size), None], nb_iter=3)
    lps = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("potts8", "random2")]
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_admm_many(lps, nb_iter=3)


# ------------------------------------------------------------------ public surface
def test_exports_and_signatures():
    for name in ("ADMMManyState", "lp_admm_many", "solve_admm_many"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name), name
    assert str(inspect.signature(lp_admm_many)) == (
        "(problems, x0=None, gamma_eq=2, gamma_ineq=3, nb_iter=100, callback_func=None, max_time=None, use_preconditioning=True, "
        "nb_iter_plot=10)")
    assert str(inspect.signature(solve_admm_many)) == "(lps, get_timing=True, nb_iter=10000, max_time=None, nb_iter_plot=10)"
    assert sparselp_module.solve_admm_many is solve_admm_many


def test_solve_many_keeps_refusing_admm(no_library):
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    with pytest.raises(ValueError, match="chambolle_pock_ppd"):
        solve_many(lps, method="admm")
    assert sparselp_module.many_methods == ("chambolle_pock_ppd",)
    assert "solve_admm_many" in solve_many.__doc__


ABI = ("create", "destroy", "iterate", "sweep_step", "multiplier_step", "report", "get_x", "get_lambda", "num_levels", "form", "lds_limit",
       "kmax", "bench")
# what stands for lines of the reference, and so cites them
CITING = ("create", "iterate", "sweep_step", "multiplier_step", "report", "get_x", "get_lambda", "num_levels", "bench")


def test_the_abi_is_declared_with_its_citations_bound_and_built():
    header = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", bare)))
    want = sorted("slp_admm_many_" + n for n in ABI)
    assert sorted(n for n in declared if n.startswith("slp_admm_many_")) == want
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_admm_many_")) == want
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared
    # every prototype stands under a comment (or carries one), and those with a counterpart in the reference cite its lines
    section = header[header.rindex("/*", 0, header.index("ADMM on a list of LPs")):]

    def comment_of(name):
        code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group()), section, flags=re.S)   # a comment may name a function too
        at = re.search(r"\b" + name + r"\s*\(", code).start()
        line_end = section.index("\n", section.index(";", at))
        before = re.findall(r"/\*.*?\*/", section[:at], flags=re.S)
        return before[-1] + " ".join(re.findall(r"/\*.*?\*/", section[at:line_end], flags=re.S))

    for n in ABI:
        text = comment_of("slp_admm_many_" + n)
        if n in CITING:
            assert re.search(r":\d+", text), f"slp_admm_many_{n} cites no line of the reference"
    assert re.search(r"ADMM\.py:\d+", comment_of("slp_admm_many_create")) and "tools.py:92" in comment_of("slp_admm_many_create")
    csrc = os.path.join(REPO, "pysparselp_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bslp_admm_many\.hip\b", makefile, flags=re.M)
    assert makefile.count("slp_admm_iter.h") == 2   # both dependency lists
    # one copy of the arithmetic: both translation units include the shared header and neither defines its functions again
    for unit in ("slp_admm_many.hip", "slp_admm_batch.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "slp_admm_iter.h"' in text
        for fn in ("admm_dot", "admm_rhs_one", "admm_sweep_one", "admm_mult_one"):
            assert not re.search(r"__device__[^;{]*\b" + fn + r"\(", text), (unit, fn)
    lib = _lib.load()   # dlopen works without a GPU
    for name in want:
        assert hasattr(lib, name), name
    assert lib.slp_admm_many_lds_limit() * 8 == 160000


# ------------------------------------------------------------------ the assembly
def _hand_made():
    """Three LPs: both kinds of rows; no equality rows; one variable and one inequality row."""
    csr = scipy.sparse.csr_matrix
    a = (np.array([1.0, -2.0, 0.5]), csr(np.array([[1.0, 0, 2.0], [0, 3.0, 0]])), np.array([4.0, 5.0]),
         csr(np.array([[0, 0, 6.0], [7.0, 8.0, 0]])), np.array([-1.0, -np.inf]), np.array([1.0, 2.0]), np.zeros(3), np.ones(3))
    b = (np.array([3.0, 4.0]), None, None, csr(np.array([[9.0, 0], [0, 0], [10.0, 11.0]])), None, np.array([5.0, 6.0, 7.0]),
         np.array([-np.inf, 0.0]), np.array([2.0, np.inf]))
    c = (np.array([-1.0]), csr(np.array([[12.0]])), np.array([0.25]), csr(np.array([[13.0]])), np.array([0.0]), np.array([np.inf]),
         np.array([-5.0]), np.array([5.0]))
    return [a, b, c]


def test_offsets_and_tables_of_a_hand_made_list():
    problems = _hand_made()
    s = admm_many_system([_admm_many_problem(k, p) for k, p in enumerate(problems)])
    for name, want in (("n", [3, 2, 1]), ("m_eq", [2, 0, 1]), ("m_ineq", [2, 3, 1]), ("col0", [0, 3, 5]), ("eq0", [0, 2, 2]),
                       ("in0", [0, 2, 5]), ("x0", [0, 5, 10]), ("lam0", [0, 4, 7])):
        assert s[name].dtype == np.int64 and np.array_equal(s[name], want), name
    for tag in ("eq", "in"):
        assert s[tag + "_indptr"].dtype == np.int64 and s[tag + "_indices"].dtype == np.int32 and s[tag + "_data"].dtype == np.float64
    # the equality rows of all LPs, then (a block of its own) the inequality rows of all LPs; columns offset by col0
    assert np.array_equal(s["eq_indptr"], [0, 2, 3, 4])
    assert np.array_equal(s["eq_indices"], [0, 2, 1, 5]) and np.array_equal(s["eq_data"], [1.0, 2.0, 3.0, 12.0])
    assert np.array_equal(s["b_eq"], [4.0, 5.0, 0.25])
    assert np.array_equal(s["in_indptr"], [0, 1, 3, 4, 4, 6, 7])
    assert np.array_equal(s["in_indices"], [2, 0, 1, 3, 3, 4, 5]) and np.array_equal(s["in_data"], [6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 13.0])
    assert np.array_equal(s["b_lower"], [-1.0, -np.inf, -np.inf, -np.inf, -np.inf, 0.0])   # an absent side: -inf / +inf
    assert np.array_equal(s["b_upper"], [1.0, 2.0, 5.0, 6.0, 7.0, np.inf])
    assert np.array_equal(s["c"], [1.0, -2.0, 0.5, 3.0, 4.0, -1.0])
    assert np.array_equal(s["lb"], [0, 0, 0, -np.inf, 0.0, -5.0]) and np.array_equal(s["ub"], [1, 1, 1, 2.0, np.inf, 5.0])
    # against scipy's block diagonals
    for tag, pos in (("eq", 1), ("in", 3)):
        blocks = [scipy.sparse.csr_matrix((0, p[0].size)) if p[pos] is None else p[pos] for p in problems]
        want = scipy.sparse.block_diag(blocks, format="csr")
        got = scipy.sparse.csr_matrix((s[tag + "_data"], s[tag + "_indices"], s[tag + "_indptr"]), shape=want.shape)
        assert (got != want).nnz == 0
    # a list without any equality row
    s = admm_many_system([_admm_many_problem(0, problems[1])])
    assert np.array_equal(s["eq_indptr"], [0]) and s["eq_indices"].size == 0 and s["b_eq"].size == 0 and s["m_eq"].sum() == 0


def test_every_row_keeps_the_entry_order_of_its_lp():
    """The sequential sums depend on it: an LP whose rows are stored in descending column order."""
    a_ineq = scipy.sparse.csr_matrix((np.array([1.0, 2.0, 3.0, 4.0]), np.array([2, 0, 1, 0], dtype=np.int32), np.array([0, 2, 4])),
                                     shape=(2, 3))
    assert not a_ineq.has_sorted_indices
    first = _hand_made()[0]
    odd = (np.ones(3), None, None, a_ineq, None, np.ones(2), np.zeros(3), np.ones(3))
    s = admm_many_system([_admm_many_problem(0, first), _admm_many_problem(1, odd)])
    q0 = s["in_indptr"][s["in0"][1]]
    assert np.array_equal(s["in_indices"][q0:] - s["col0"][1], [2, 0, 1, 0]) and np.array_equal(s["in_data"][q0:], [1.0, 2.0, 3.0, 4.0])


def test_the_composite_gives_every_lp_the_bits_of_its_own_solve():
    """``oracle.lp_admm`` -- row scalings, standard form, second scaling, M, A^T b, 37 iterations -- on the arguments built for
    SC50A + Potts-8 + random0 + SC105 as ONE LP returns, per LP, the bits of ``oracle.lp_admm`` on that LP alone."""
    from oracle import oracle

    cases = ["sc50a", "potts8", "random0", "sc105"]
    problems = [solver_args(load_golden("lp_" + c)) for c in cases]
    assert any(p[4] is None for p in problems) and any(p[4] is not None for p in problems) and any(p[1] is None for p in problems)
    s = admm_many_system([_admm_many_problem(k, p) for k, p in enumerate(problems)])
    n, m_eq, m_in = int(s["n"].sum()), int(s["m_eq"].sum()), int(s["m_ineq"].sum())
    a_eq = scipy.sparse.csr_matrix((s["eq_data"], s["eq_indices"], s["eq_indptr"]), shape=(m_eq, n))
    a_ineq = scipy.sparse.csr_matrix((s["in_data"], s["in_indices"], s["in_indptr"]), shape=(m_in, n))
    last = {}

    def hook(i, x, x_all, lambda_eq):
        last["x"], last["lam"] = x_all.copy(), lambda_eq.copy()

    x = oracle.lp_admm(s["c"], a_eq, s["b_eq"], a_ineq, s["b_lower"], s["b_upper"], s["lb"], s["ub"], nb_iter=37, nb_iter_plot=100,
                       iterate_hook=hook)
    for k, p in enumerate(problems):
        own = {}

        def own_hook(i, x, x_all, lambda_eq, own=own):
            own["x"], own["lam"] = x_all.copy(), lambda_eq.copy()

        want = oracle.lp_admm(*p, nb_iter=37, nb_iter_plot=100, iterate_hook=own_hook)
        c0, nk, me, mi, e0, i0 = (int(s[name][k]) for name in ("col0", "n", "m_eq", "m_ineq", "eq0", "in0"))
        assert np.array_equal(x[c0:c0 + nk], want), cases[k]
        # the slacks and the multipliers too: the LP's own order is variables, then its slacks; equality rows, then its inequality rows
        assert np.array_equal(np.concatenate((last["x"][c0:c0 + nk], last["x"][n + i0:n + i0 + mi])), own["x"]), cases[k]
        assert np.array_equal(np.concatenate((last["lam"][e0:e0 + me], last["lam"][m_eq + i0:m_eq + i0 + mi])), own["lam"]), cases[k]
