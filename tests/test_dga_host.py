"""Dual gradient ascent (reference DualGradientAscent.py:36-245) without a GPU: the numpy restatement tests/dga_cpu.py against
the reference's results in tests/golden/dga.npz, its re-ordered forms inside each case's agreement horizon, and the public
surface (method name, refused inputs, C ABI names)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, csr_of, load_golden, lp_from_golden
from dga_cpu import dga_cpu

CASES = ("sc50a", "sc105", "potts8", "potts50", "random0", "random1", "random2")
# at least 1000 iterations on the small cases, 100 on SC105, 200 on Potts-50: what the recorded horizons must reach
REQUIRED_HORIZON = {"sc50a": 1000, "potts8": 1000, "random0": 1000, "random1": 1000, "random2": 1000, "sc105": 100, "potts50": 200}


def dga_args(d):
    """(c, a_eq, b_eq, a_ineq, b_upper, lb, ub) of a fixture LP as dga_cpu takes them."""
    ai = csr_of(d, "Ai")
    return d["c"], csr_of(d, "Ae"), d["be"], (ai if ai.shape[0] > 0 else None), d["bu"], d["lb"], d["ub"]


def same_state(got, x, y_eq, y_ineq, draws):
    ok = np.array_equal(got[0], x) and np.array_equal(got[1], y_eq) and got[3] == draws
    return ok and (np.array_equal(got[2], y_ineq) if got[2] is not None else y_ineq.size == 0)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_bit_for_bit(case):
    g = load_golden("dga")
    keep = [int(i) for i in g[f"{case}_it"]]
    got = dga_cpu(*dga_args(load_golden("lp_" + case)), nb_max_iter=max(keep) + 1, order="reference", keep=keep)
    for k, it in enumerate(keep):
        assert same_state(got[it], g[f"{case}_x"][k], g[f"{case}_yeq"][k], g[f"{case}_yineq"][k], int(g[f"{case}_draws"][k])), it


@pytest.mark.parametrize("order,block", [("blocked", 16), ("blocked", 64), ("blocked", 256), ("device", 0)])
@pytest.mark.parametrize("case", CASES)
def test_reordered_sums_agree_inside_the_horizon(case, order, block):
    g = load_golden("dga")
    horizon = int(g[f"{case}_horizon"])
    assert horizon >= REQUIRED_HORIZON[case]
    keep = [int(i) for i in g[f"{case}_it"] if i <= horizon]
    got = dga_cpu(*dga_args(load_golden("lp_" + case)), nb_max_iter=horizon + 1, order=order, block=block, keep=keep)
    for k, it in enumerate(keep):
        assert same_state(got[it], g[f"{case}_x"][k], g[f"{case}_yeq"][k], g[f"{case}_yineq"][k], int(g[f"{case}_draws"][k])), it


def test_fixture_exercises_the_tie_rule():
    g = load_golden("dga")
    with_ties = 0
    for case in CASES:
        keep = [int(i) for i in g[f"{case}_it"]]
        with_ties += int(g[f"{case}_draws"][keep.index(int(g[f"{case}_horizon"]))]) > 0
    assert with_ties >= 3


def test_solving_methods_is_unchanged_and_dual_methods_is_new():
    from pysparselp_amd import SparseLP

    assert SparseLP.solving_methods == ("chambolle_pock_ppd", "admm", "admm_blocks", "admm2")
    assert SparseLP.dual_methods == ("dual_gradient_ascent",)


@pytest.mark.parametrize("fixture", ["ka_l1svm", "ka_kmedians"])
def test_solve_knows_the_method_and_refuses_finite_b_lower_before_loading_the_library(monkeypatch, fixture):
    from pysparselp_amd import _lib
    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent
    from pysparselp_amd.SparseLP import SparseLP

    def loaded(*a, **k):
        raise RuntimeError("the library was asked for")

    monkeypatch.setattr(_lib, "load", loaded)
    monkeypatch.setattr(_lib, "lib", loaded)
    lp = lp_from_golden(load_golden(fixture), SparseLP)
    assert lp.b_lower is not None and np.max(lp.b_lower) > -np.inf
    with pytest.raises(ValueError, match="b_lower"):
        lp.solve(method="dual_gradient_ascent", nb_iter=10)
    with pytest.raises(ValueError, match="b_lower"):
        dual_gradient_ascent(None, lp, nb_max_iter=10)
    with pytest.raises(ValueError, match="dual_gradient_ascent") as e:
        lp.solve(method="no_such_method")
    assert "admm2" in str(e.value)
    # an LP it accepts gets as far as the library
    ok = lp_from_golden(load_golden("lp_sc50a"), SparseLP)
    with pytest.raises(RuntimeError, match="the library was asked for"):
        ok.solve(method="dual_gradient_ascent", nb_iter=10)


def test_dual_gradient_ascent_signature_is_the_reference_one():
    import inspect

    from pysparselp_amd.DualGradientAscent import dual_gradient_ascent, exact_dual_line_search

    e = inspect.Parameter.empty
    params = [(p.name, p.default) for p in inspect.signature(dual_gradient_ascent).parameters.values()]
    assert params == [("x", e), ("lp", e), ("nb_max_iter", 1000), ("callback_func", None), ("y_eq", None), ("y_ineq", None),
                      ("max_time", None), ("nb_iter_plot", 1)]
    names = list(inspect.signature(exact_dual_line_search).parameters)
    assert names[:6] == ["direction", "a", "b", "c_bar", "upper_bounds", "lower_bounds"]


def test_c_abi_names_are_declared_in_the_header_and_in_the_binding():
    from pysparselp_amd import _lib

    names = ("slp_dga_create_on", "slp_dga_destroy", "slp_dga_iterate", "slp_dga_get_x", "slp_dga_get_y", "slp_dga_report",
             "slp_dga_push_random", "slp_dga_status", "slp_dga_line_search", "slp_dga_set_path", "slp_dga_path",
             "slp_dga_iterations", "slp_dga_timing", "slp_dga_timing_read")
    header = open(os.path.join(REPO, "include", "slp_hip.h")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("slp_dga_")) == sorted(names)
    makefile = open(os.path.join(REPO, "pysparselp_amd", "csrc", "Makefile")).read()
    assert "slp_dga.hip" in makefile
