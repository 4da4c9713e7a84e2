"""Host logic of dual gradient ascent on a list of LPs (``dual_gradient_ascent_many``, ``DeviceDGAMany``,
``SparseLP.solve_dga_many``): every refusal comes before the library is touched, the assembled system (rows LP by LP, indices
local to their LP, per-LP table) and the draw offsets are the ones the device expects, and the C ABI is declared, bound and
built.  None of it needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse

from conftest import REPO, load_golden, lp_from_golden
from dga_many_cases import LP, extra_list, mixed_list, rows_of
from pysparselp_amd import SparseLP as sparselp_module
from pysparselp_amd import _lib, dual_gradient_ascent_many, solve_dga_many
from pysparselp_amd.DualGradientAscent import FUSED_MAX, _dga_many_lp, dga_many_start, dga_many_system
from pysparselp_amd.SparseLP import SparseLP

NAMES = ("create", "destroy", "iterate", "push_random", "status", "frozen", "get_x", "get_y", "report", "timing", "timing_read", "kmax")


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load or bind the library fails the test: validation must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _lps():
    return [LP(*args) for _, _, args in mixed_list()[:4]]   # potts8 (inequalities only), random0, random1, sc50a


def _changed(lp, **changes):
    out = LP(lp.costsvector, lp.a_equalities, lp.b_equalities, lp.a_inequalities, lp.b_upper, lp.lower_bounds, lp.upper_bounds, lp.b_lower)
    for name, v in changes.items():
        setattr(out, name, v)
    return out


def test_an_empty_list_is_refused(no_library):
    with pytest.raises(ValueError, match="empty list"):
        dual_gradient_ascent_many([])
    with pytest.raises(ValueError, match="empty list"):
        solve_dga_many([])
    with pytest.raises(ValueError, match="sequence of LP objects"):
        dual_gradient_ascent_many(None)
    with pytest.raises(ValueError, match="LP 1 is not an LP object"):
        dual_gradient_ascent_many([_lps()[0], 3.0])


def test_a_finite_b_lower_is_refused_and_names_the_lp(no_library):
    lps = _lps()
    m_in = lps[3].a_inequalities.shape[0]
    lps[3] = _changed(lps[3], b_lower=np.full(m_in, -1.0))
    with pytest.raises(ValueError, match="LP 3: .*one-sided inequalities"):
        dual_gradient_ascent_many(lps)
    lps[3] = _changed(lps[3], b_lower=np.full(m_in, -np.inf))   # all -inf is one-sided
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many(lps, nb_max_iter=2)
    sp = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("potts8", "sc50a")]
    sp[1].b_lower = np.zeros(sp[1].a_inequalities.shape[0])
    with pytest.raises(ValueError, match="LP 1: .*one-sided inequalities"):
        solve_dga_many(sp, nb_iter=3)


def test_shape_errors_are_refused_and_name_the_lp(no_library):
    lps = _lps()
    p = lps[3]   # sc50a: both kinds of rows
    n, (m_eq, m_in) = p.costsvector.size, (p.a_equalities.shape[0], p.a_inequalities.shape[0])
    wrong = scipy.sparse.csr_matrix(p.a_inequalities)
    wrong.indices = wrong.indices.copy()
    wrong.indices[2] = n
    bad = [
        ("costsvector has shape", _changed(p, costsvector=np.zeros((2, n)))),
        ("costsvector has shape", _changed(p, costsvector=np.zeros(0))),
        ("a_equalities has .* columns", _changed(p, costsvector=p.costsvector[:-1], lower_bounds=p.lower_bounds[:-1], upper_bounds=p.upper_bounds[:-1])),
        ("lower_bounds has shape", _changed(p, lower_bounds=p.lower_bounds[:-1])),
        ("upper_bounds has shape", _changed(p, upper_bounds=np.zeros(n + 1))),
        ("b_equalities has shape", _changed(p, b_equalities=np.zeros(m_eq + 1))),
        ("b_upper has shape", _changed(p, b_upper=np.zeros(m_in - 1))),
        ("a_inequalities has a column index outside", _changed(p, a_inequalities=wrong)),
    ]
    for match, lp in bad:
        with pytest.raises(ValueError, match="LP 2: " + match):
            dual_gradient_ascent_many([lps[0], lps[1], lp])
    with pytest.raises(ValueError, match="y_eq must be None or a sequence of 4"):
        dual_gradient_ascent_many(lps, y_eq=[None, None])
    with pytest.raises(ValueError, match="y_ineq must be None or a sequence of 4"):
        dual_gradient_ascent_many(lps, y_ineq=0.5)
    with pytest.raises(ValueError, match="LP 3: y_eq has shape"):
        dual_gradient_ascent_many(lps, y_eq=[None, None, None, np.zeros(m_eq + 1)])
    with pytest.raises(ValueError, match="LP 0: y_ineq has shape"):
        dual_gradient_ascent_many(lps, y_ineq=[np.zeros(3), None, None, None])


def test_an_lp_without_rows_or_with_too_many_variables_is_refused(no_library):
    lps = _lps()
    p = lps[1]
    n = p.costsvector.size
    for rowless in (_changed(p, a_equalities=scipy.sparse.csr_matrix((0, n)), b_equalities=np.zeros(0), a_inequalities=None, b_upper=None),
                    _changed(p, a_equalities=None, b_equalities=None, a_inequalities=scipy.sparse.csr_matrix((0, n)), b_upper=np.zeros(0))):
        with pytest.raises(ValueError, match="LP 1 has no constraint rows"):
            dual_gradient_ascent_many([lps[0], rowless, lps[2]])
    big = FUSED_MAX + 1
    assert FUSED_MAX == 8192
    wide = LP(np.ones(big), scipy.sparse.csr_matrix((np.ones(1), np.array([big - 1]), np.array([0, 1])), shape=(1, big)), np.ones(1), None, None,
              np.zeros(big), np.ones(big))
    with pytest.raises(ValueError, match="LP 2 has 8193 variables.*at most 8192.*single solver"):
        dual_gradient_ascent_many([lps[0], lps[1], wide])
    # 8192 variables are taken
    fits = LP(np.ones(FUSED_MAX), scipy.sparse.csr_matrix((np.ones(1), np.array([5]), np.array([0, 1])), shape=(1, FUSED_MAX)), np.ones(1), None,
              None, np.zeros(FUSED_MAX), np.ones(FUSED_MAX))
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many([fits])


def test_an_accepted_call_gets_as_far_as_the_library(no_library):
    lps = _lps()
    with pytest.raises(AssertionError, match="library was loaded"):
        dual_gradient_ascent_many(lps, nb_max_iter=3, y_eq=[None, np.zeros(lps[1].a_equalities.shape[0]), None, None])
    sp = [lp_from_golden(load_golden("lp_" + c), SparseLP) for c in ("potts8", "sc50a")]
    with pytest.raises(AssertionError, match="library was loaded"):
        solve_dga_many(sp, nb_iter=3)


def test_signatures_and_exports():
    import pysparselp_amd

    assert str(inspect.signature(dual_gradient_ascent_many)) == "(lps, nb_max_iter=1000, callback_func=None, y_eq=None, y_ineq=None, max_time=None)"
    assert str(inspect.signature(solve_dga_many)) == "(lps, get_timing=True, nb_iter=10000, max_time=None)"
    assert str(inspect.signature(pysparselp_amd.DeviceDGAMany.__init__)) == "(self, lps, y0s, draw_offsets, draws=None)"
    assert sparselp_module.solve_dga_many is solve_dga_many
    for name in ("DeviceDGAMany", "dual_gradient_ascent_many", "solve_dga_many"):
        assert name in pysparselp_amd.__all__ and hasattr(pysparselp_amd, name)
    for name in ("iterate", "status", "frozen", "check", "x", "y", "report", "close"):
        assert callable(getattr(pysparselp_amd.DeviceDGAMany, name)), name


def test_solve_many_and_the_pinned_tuples_stay(no_library):
    lps = [lp_from_golden(load_golden("lp_potts8"), SparseLP)]
    with pytest.raises(ValueError, match="chambolle_pock_ppd"):
        sparselp_module.solve_many(lps, method="dual_gradient_ascent")
    assert sparselp_module.many_methods == ("chambolle_pock_ppd",)
    assert sparselp_module.solving_methods == ("chambolle_pock_ppd", "admm", "admm_blocks", "admm2")
    assert sparselp_module.dual_methods == ("dual_gradient_ascent",)
    assert sparselp_module.batch_methods == ("chambolle_pock_ppd",)


def _all_args():
    return [args for _, _, args in mixed_list()] + [args for _, args in extra_list()]


def test_the_assembly_is_the_block_diagonal_of_the_single_systems():
    problems = _all_args()
    assert any(rows_of(a)[0] == 0 for a in problems) and any(rows_of(a)[1] == 0 for a in problems)   # both one-kind forms are in
    forms = [_dga_many_lp(k, LP(*a)) for k, a in enumerate(problems)]
    y0s, offsets = dga_many_start(forms)
    s = dga_many_system(forms, y0s, offsets)
    n = np.array([a[0].size for a in problems])
    m_eq = np.array([rows_of(a)[0] for a in problems])
    m_in = np.array([rows_of(a)[1] for a in problems])
    m = m_eq + m_in
    assert np.array_equal(s["n"], n) and np.array_equal(s["m_eq"], m_eq) and np.array_equal(s["m_ineq"], m_in)
    assert np.array_equal(s["col0"], np.concatenate(([0], np.cumsum(n)[:-1])))
    assert np.array_equal(s["row0"], np.concatenate(([0], np.cumsum(m)[:-1])))
    for name, dtype in (("n", np.int64), ("m_eq", np.int64), ("m_ineq", np.int64), ("draw_offset", np.int64), ("indptr", np.int64),
                        ("indices", np.int32), ("data", np.float64), ("b", np.float64), ("y0", np.float64), ("c", np.float64)):
        assert s[name].dtype == dtype and s[name].flags.c_contiguous, name
    singles = []
    for a in problems:
        blocks = [scipy.sparse.csr_matrix(blk) for blk in (a[1], a[3]) if blk is not None and blk.shape[0] > 0]
        singles.append(scipy.sparse.vstack(blocks).tocsr() if len(blocks) > 1 else blocks[0])
    # K: the indices are local; offset by col0 they give scipy's block diagonal
    cols = s["indices"].astype(np.int64) + np.repeat(np.repeat(s["col0"], m), np.diff(s["indptr"]))
    k_all = scipy.sparse.csr_matrix((s["data"], cols, s["indptr"]), shape=(int(m.sum()), int(n.sum())))
    want = scipy.sparse.block_diag(singles, format="csr")
    assert (k_all != want).nnz == 0 and k_all.nnz == sum(blk.nnz for blk in singles) == s["indptr"][-1]
    for k, own in enumerate(singles):
        q0, q1 = s["indptr"][s["row0"][k]], s["indptr"][s["row0"][k] + m[k]]
        assert s["indices"][q0:q1].min() >= 0 and s["indices"][q0:q1].max() < n[k]
        # every row keeps the entry order of its LP's own matrix (the sequential sums depend on it)
        assert np.array_equal(s["indptr"][s["row0"][k]:s["row0"][k] + m[k] + 1] - q0, own.indptr)
        assert np.array_equal(s["indices"][q0:q1], own.indices) and np.array_equal(s["data"][q0:q1], own.data)
    b = [np.concatenate((a[2] if rows_of(a)[0] else np.zeros(0), a[4] if rows_of(a)[1] else np.zeros(0))) for a in problems]
    assert np.array_equal(s["b"], np.concatenate(b))
    for name, pos in (("c", 0), ("lb", 5), ("ub", 6)):
        assert np.array_equal(s[name], np.concatenate([a[pos] for a in problems]))
    assert np.array_equal(s["y0"], np.concatenate(y0s))


def test_draw_offsets_of_default_given_and_mixed_starts():
    problems = _all_args()[:4]
    forms = [_dga_many_lp(k, LP(*a)) for k, a in enumerate(problems)]
    shapes = [rows_of(a) for a in problems]
    # default: the reference's seed-0 start of the LP's own shape; the tie draws continue behind it
    y0s, offsets = dga_many_start(forms)
    assert offsets == [me + mi for me, mi in shapes]
    for (me, mi), y0 in zip(shapes, y0s):
        rs = np.random.RandomState(0)
        assert np.array_equal(y0[:me], -rs.rand(me)) and np.array_equal(y0[me:], np.abs(rs.rand(mi)))
        assert np.all(y0[:me] <= 0) and np.all(y0[me:] >= 0)
    # given: nothing is drawn
    rs = np.random.RandomState(9)
    ye = [rs.randn(me) for me, _ in shapes]
    yi = [rs.rand(mi) for _, mi in shapes]
    y0s, offsets = dga_many_start(forms, ye, yi)
    assert offsets == [0, 0, 0, 0]
    for k in range(4):
        assert np.array_equal(y0s[k], np.concatenate((ye[k], yi[k])))
    y0s[0][:] = 7.0
    assert not np.any(yi[0] == 7.0)   # copies
    # mixed: only the parts that are drawn count, and a drawn y_ineq then starts the stream
    y0s, offsets = dga_many_start(forms, [None, ye[1], None, ye[3]], [None, None, yi[2], yi[3]])
    assert offsets == [sum(shapes[0]), shapes[1][1], shapes[2][0], 0]
    assert np.array_equal(y0s[1], np.concatenate((ye[1], np.abs(np.random.RandomState(0).rand(shapes[1][1])))))
    assert np.array_equal(y0s[2], np.concatenate((-np.random.RandomState(0).rand(shapes[2][0]), yi[2])))
    s = dga_many_system(forms, y0s, offsets)
    assert np.array_equal(s["draw_offset"], offsets)


def _header_functions():
    text = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(slp_[a-z0-9_]+)\s*\(", text)))


def test_the_abi_is_declared_bound_and_built():
    declared = _header_functions()
    want = sorted("slp_many_dga_" + n for n in NAMES)
    assert sorted(n for n in declared if n.startswith("slp_many_dga_")) == want
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_many_dga_")) == want
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared
    csrc = os.path.join(REPO, "pysparselp_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bslp_dga_many\.hip\b", makefile, flags=re.M)
    for unit in ("slp_dga_many.hip", "slp_dga.hip", "slp_dga_batch.hip"):   # one set of bodies for all three
        assert '#include "slp_dga_shared.h"' in open(os.path.join(csrc, unit)).read(), unit
    lib = _lib.load()   # dlopen works without a GPU
    for name in want:
        assert hasattr(lib, name), name
