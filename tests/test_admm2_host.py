"""lp_admm2 (reference ADMM.py:272-474) without a GPU: the public surface, and a numpy restatement of the matrix-free form
the device runs (csrc/slp_blocks.hip, slp_admm2_*) against the reference's LU iterates in tests/golden/admm2.npz."""
import inspect

import numpy as np
import pytest
import scipy.sparse

from conftest import load_golden, solver_args

CASES = {"sc50a": "lp_sc50a", "sc105": "lp_sc105", "potts8": "lp_potts8", "potts50": "lp_potts50", "random0": "lp_random0",
         "random1": "lp_random1", "random2": "lp_random2", "l1svm": "ka_l1svm", "sc105_pre": "lp_sc105"}


def admm2_matrix_free(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, nb_iter, callback, use_preconditioning=False, gamma=0.7,
                      alpha=1.95, tol=1e-13, max_steps=500):
    """lp_admm2 with x0 = 0 whose KKT solve is the projection of v = (-c + gamma xp - lambda) / gamma onto {A x = b}: conjugate
    gradients on A A^T + [0; I] over the rows (slack column implicit), from the previous multiplier."""
    from pysparselp_amd.tools import convert_to_standard_form_with_bounds, precondition_constraints

    n = c.size
    if use_preconditioning:  # ADMM.py:308-329: every row of the explicit standard form an equality
        a_eq, beq = precondition_constraints(a_eq, beq, alpha=2)
        a_ineq, b_lower, b_upper = precondition_constraints(a_ineq, b_lower, b_upper, alpha=2)
        c, a, b, lb, ub, _ = convert_to_standard_form_with_bounds(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, np.zeros(n))
        a, b = precondition_constraints(a, b, alpha=2)
        a, m_eq, slo, shi = a.tocsr(), a.shape[0], np.zeros(0), np.zeros(0)
    else:
        m_eq = 0 if a_eq is None else a_eq.shape[0]
        a = scipy.sparse.vstack([blk for blk in (a_eq, a_ineq) if blk is not None]).tocsr()
        b = np.concatenate((np.zeros(0) if a_eq is None else beq, np.zeros(a_ineq.shape[0])))
        slo = np.full(a_ineq.shape[0], -np.inf) if b_lower is None else b_lower
        shi = np.full(a_ineq.shape[0], np.inf) if b_upper is None else b_upper
    m, ineq = a.shape[0], np.arange(a.shape[0]) >= m_eq
    xp, xps = np.clip(np.zeros(c.size), lb, ub), np.clip(np.zeros(m - m_eq), slo, shi)
    lam, lams, nu = np.zeros(c.size), np.zeros(m - m_eq), np.zeros(m)
    apply = lambda p: a @ (a.T @ p) + ineq * p  # noqa: E731
    for it in range(nb_iter + 1):
        v, vs = (-c + gamma * xp - lam) / gamma, xps - lams / gamma
        rhs = a @ v - np.concatenate((np.zeros(m_eq), vs)) - b
        r = rhs - apply(nu)
        d, rs = r.copy(), r @ r
        for _ in range(max_steps):
            if not rs > tol * tol * (rhs @ rhs):
                break
            q = apply(d)
            step = rs / (d @ q)
            nu, r = nu + step * d, r - step * q
            rs, rs_old = r @ r, rs
            d = r + (rs / rs_old) * d
        x = alpha * (v - a.T @ nu) + (1 - alpha) * xp
        xs = alpha * (vs + nu[m_eq:]) + (1 - alpha) * xps
        xp, xps = np.clip(x + lam / gamma, lb, ub), np.clip(xs + lams / gamma, slo, shi)
        energy = c @ x + 0.5 * gamma * (np.sum((x - xp) ** 2) + np.sum((xs - xps) ** 2)) + lam @ (x - xp) + lams @ (xs - xps)
        callback(it, x[:n], energy)
        lam, lams = lam + gamma * (x - xp), lams + gamma * (xs - xps)
    return x[:n]


def test_admm2_is_a_solving_method():
    from pysparselp_amd.SparseLP import solving_methods

    assert solving_methods[:3] == ("chambolle_pock_ppd", "admm", "admm_blocks")
    assert solving_methods[3:] == ("admm2",)


def test_lp_admm2_signature_is_the_reference_one():
    from pysparselp_amd.ADMM import lp_admm2

    params = [(p.name, p.default) for p in inspect.signature(lp_admm2).parameters.values()]
    e = inspect.Parameter.empty
    assert params == [("c", e), ("a_eq", e), ("beq", e), ("a_ineq", e), ("b_lower", e), ("b_upper", e), ("lb", e), ("ub", e),
                      ("x0", None), ("gamma_ineq", 0.7), ("nb_iter", 100), ("callback_func", None), ("max_time", None),
                      ("use_preconditioning", False), ("nb_iter_plot", 10), ("cg_tol", 1e-13), ("cg_max_steps", 500)]


def test_lp_admm2_refuses_what_the_reference_cannot_run(monkeypatch):
    """No inequality block: the reference's UnboundLocalError (tools.py:92-127).  use_preconditioning on an LP that needs row
    chunks: a ValueError before anything reaches the device."""
    from pysparselp_amd.ADMM import lp_admm2

    c, a_eq, beq, a_ineq, bl, bu, lb, ub = solver_args(load_golden("lp_sc105"))
    with pytest.raises(UnboundLocalError):
        lp_admm2(c, a_eq, beq, None, None, None, lb, ub)
    monkeypatch.setenv("SLP_SETUP_CHUNK_ENTRIES", "100")
    with pytest.raises(ValueError, match="chunks"):
        lp_admm2(c, a_eq, beq, a_ineq, bl, bu, lb, ub, use_preconditioning=True)


@pytest.mark.parametrize("case", list(CASES))
def test_matrix_free_restatement_reproduces_the_reference_lu_iterates(case):
    g = load_golden("admm2")
    d = load_golden(CASES[case])
    ref = {int(i): (x, e) for i, x, e in zip(g[f"{case}_it"], g[f"{case}_x"], g[f"{case}_e1"])}
    got = {}

    def cb(it, x, energy):
        if it in ref:
            got[it] = (x.copy(), energy)

    admm2_matrix_free(*solver_args(d), nb_iter=max(ref), callback=cb, use_preconditioning=case.endswith("_pre"))
    assert sorted(got) == sorted(ref)
    for it, (x, e) in ref.items():
        assert np.max(np.abs(got[it][0] - x) / (1 + np.abs(x))) < 1e-9, it
        np.testing.assert_allclose(got[it][1], e, rtol=1e-7)
