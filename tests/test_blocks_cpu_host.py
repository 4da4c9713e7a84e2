"""tests/blocks_cpu.py -- the exact reference of the matrix-free projection solvers -- without a GPU, against what the project
already trusts: the reference's LU iterates of lp_admm2 (tests/golden/admm2.npz, ``_admm2_lu``), ``oracle.lp_admm_block_decomposition``
with one block, and a dense KKT solve with a starting point.  Then what tests/test_gpu_projection_edges.py and
tests/test_gpu_fuzz_projection.py rely on: every edge case's system is regular (lambda_min > 0, condition <= 1e6) in the form the
device takes, the step-limit case needs more conjugate-gradient steps than its largest cap, and the fuzz generator throws away
no more than a fifth of its draws for the seed the GPU test uses."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse

import blocks_cases
import blocks_cpu
from conftest import Recorder, load_golden, solver_args
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_projection  # noqa: E402

GOLDEN_LPS = ["potts8", "sc50a", "random0"]


def _stacked(args):
    """solver_args -> the device's layout: (a, m_eq, b_lower, b_upper, c, lb, ub)."""
    c, a_eq, beq, a_ineq, bl, bu, lb, ub = args
    m_eq = 0 if a_eq is None else a_eq.shape[0]
    a = scipy.sparse.vstack([blk for blk in (a_eq, a_ineq) if blk is not None]).tocsr()
    beq = np.zeros(0) if a_eq is None else beq
    bl = np.full(a_ineq.shape[0], -np.inf) if bl is None else bl
    return a, m_eq, np.concatenate((beq, bl)), np.concatenate((beq, bu)), c, lb, ub


def _rel(x, ref):
    return float(np.max(np.abs(x - ref) / (1 + np.abs(ref))))


@pytest.mark.parametrize("name", GOLDEN_LPS)
def test_admm2_exact_reproduces_the_reference_lu_iterates(name):
    g = load_golden("admm2")
    ref = {int(i): (x, e) for i, x, e in zip(g[f"{name}_it"], g[f"{name}_x"], g[f"{name}_e1"])}
    xs, es = blocks_cpu.admm2_exact(*_stacked(solver_args(load_golden("lp_" + name))), nb_iter=max(ref) + 1)
    for it, (x, e) in ref.items():
        assert _rel(xs[it], x) < 1e-9, it
        np.testing.assert_allclose(es[it], e, rtol=1e-7)


@pytest.mark.parametrize("name", ["dual_both_kinds", "primal_natural", "empty_columns_and_rows"])
def test_admm2_exact_matches_the_sparse_lu_loop_on_edge_cases(name):
    from test_gpu_admm2 import _admm2_lu

    case = blocks_cases.case(name)
    xs, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=8)
    assert _rel(xs[-1], _admm2_lu(*blocks_cases.solver_args_of(case), nb_iter=7)) < 1e-9


def _admm2_dense_kkt(case, nb_iter, gamma=0.7, alpha=1.95):
    """ADMM.py:320-474 on the explicit standard form with a dense KKT solve, from ``x0`` (slacks ``A_in x0``, tools.py:123-124)."""
    a, m_eq, n = case["a"].toarray(), case["m_eq"], case["c"].size
    m = a.shape[0]
    mi = m - m_eq
    std = np.hstack((a, np.vstack((np.zeros((m_eq, mi)), -np.eye(mi)))))
    big = n + mi
    kkt = np.block([[gamma * np.eye(big), std.T], [std, np.zeros((m, m))]])
    cc, lo, hi = np.concatenate((case["c"], np.zeros(mi))), np.concatenate((case["lb"], case["b_lower"][m_eq:])), \
        np.concatenate((case["ub"], case["b_upper"][m_eq:]))
    b = np.concatenate((case["b_upper"][:m_eq], np.zeros(mi)))
    x = np.concatenate((case["x0"], a[m_eq:] @ case["x0"]))
    xp, lam, out = np.clip(x, lo, hi), np.zeros(big), []
    for _ in range(nb_iter):
        x = alpha * np.linalg.solve(kkt, np.concatenate((-cc + gamma * xp - lam, b)))[:big] + (1 - alpha) * xp
        xp = np.clip(x + lam / gamma, lo, hi)
        lam = lam + gamma * (x - xp)
        out.append(x[:n])
    return out


@pytest.mark.parametrize("name", ["dual_both_kinds", "one_slack", "primal_forced"])
def test_admm2_exact_with_a_starting_point_matches_a_dense_kkt_solve(name):
    case = blocks_cases.case(name)
    primal = blocks_cpu.device_primal(*case["a"].shape, case["m_eq"], case["forced"])
    xs, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=6, x0=case["x0"], primal=primal)
    for it, x in enumerate(_admm2_dense_kkt(case, 6)):
        assert _rel(xs[it], x) < 1e-9, it
    zero, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=1, primal=primal)
    assert _rel(xs[0], zero[0]) > 1e-3   # (the starting point matters)


def test_the_conjugate_gradient_projector_gives_the_exact_iterates():
    """``CgProjector`` plugged into ``admm2_exact`` is ``admm2_matrix_free`` with a starting point: what the one case without an exact
    reference is compared with."""
    from test_admm2_host import admm2_matrix_free

    case = blocks_cases.case("dual_both_kinds")
    a, m_eq = case["a"], case["m_eq"]
    b = np.concatenate((case["b_upper"][:m_eq], np.zeros(a.shape[0] - m_eq)))
    for x0 in (case["x0"], None):
        exact, ee = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=5, x0=x0)
        cg, ec = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=5, x0=x0, project=blocks_cpu.CgProjector(a, m_eq, b))
        for it in range(5):
            assert _rel(cg[it], exact[it]) < 1e-9
        np.testing.assert_allclose(ec, ee, rtol=1e-7)
    got = []
    admm2_matrix_free(*blocks_cases.solver_args_of(case), nb_iter=4, callback=lambda it, x, e: got.append(x.copy()))
    for it in range(5):   # (x0 = None was the last run: the restatement it generalises, step for step)
        assert _rel(got[it], cg[it]) < 1e-12


@pytest.mark.parametrize("name", GOLDEN_LPS + ["dual_both_kinds", "empty_columns_and_rows", "open_box", "all_equalities"])
def test_blocks_exact_matches_the_oracle_with_one_block(name):
    if name in GOLDEN_LPS:
        args = solver_args(load_golden("lp_" + name))
        stacked = _stacked(args)
    else:
        case = blocks_cases.case(name)
        args, stacked = blocks_cases.solver_args_of(case), blocks_cases.lp_args(case)
    m = stacked[0].shape[0]
    rec = Recorder()
    oracle.lp_admm_block_decomposition(*args, nb_iter=7, nb_iter_plot=1, callback_func=rec, blocks_eq=[(0, m - 1)], blocks_ineq=[])
    xs, es = blocks_cpu.blocks_exact(*stacked, nb_iter=8)
    assert rec.it == list(range(8))
    for it in range(8):
        assert _rel(xs[it], rec.x[it]) < 1e-9, it
    np.testing.assert_allclose(es, rec.e1, rtol=1e-7, atol=1e-7)
    if name == "empty_columns_and_rows":   # the unused-column rule moves them: -c / gamma per iteration until a bound stops them
        cols = blocks_cases.case(name)["empty_cols"]
        assert np.any(xs[0][cols] != xs[1][cols]) and np.any(xs[6][cols] == xs[7][cols])


@pytest.mark.parametrize("name", blocks_cases.EXACT)
def test_every_edge_case_has_a_regular_system_in_the_form_the_device_takes(name):
    case = blocks_cases.case(name)
    a, m_eq = case["a"], case["m_eq"]
    m, n = a.shape
    b = np.concatenate((case["b_upper"][:m_eq], np.zeros(m - m_eq)))
    proj = blocks_cpu.ExactProjector(a, m_eq, b, blocks_cpu.device_primal(m, n, m_eq, case["forced"]))
    print(f"{name}: {m} x {n}, m_eq {m_eq}, nnz {a.nnz}, primal {proj.primal}, lambda_min {proj.lambda_min:.3g}, "
          f"condition {proj.condition:.3g}, sigma_max {proj.sigma_max:.3g}")
    assert proj.lambda_min > 0 and proj.condition <= 1e6
    assert not np.any(np.diff(a.indptr)[:m_eq] == 0) and not np.any(a.data == 0.0)
    assert np.array_equal(a.data, np.round(a.data, 2))
    # the projection is one: feasible, and the step to it orthogonal to the constraint set's directions
    rng = np.random.RandomState(0)
    v, vs = rng.randn(n), rng.randn(m - m_eq)
    p = proj.project(v, vs)
    scale = 1 + np.abs(a) @ np.abs(p.x)
    assert np.max(np.abs(a @ p.x - np.concatenate((b[:m_eq], p.s))) / scale) < 1e-13
    assert np.max(np.abs((v - p.x) - a.T @ p.nu)) < 1e-12 * (1 + np.max(np.abs(v))) * max(1.0, proj.sigma_max)
    assert np.all(np.abs((p.s - vs) - p.nu[m_eq:]) < 1e-12 * (1 + np.max(np.abs(p.nu))))
    # the two forms of the system give the same projection
    other = blocks_cpu.project_exact(a, m_eq, b, v, vs, primal=not proj.primal) if m_eq == 0 and max(m, n) <= blocks_cpu.DENSE_LIMIT else p
    assert _rel(other.x, p.x) < 1e-12


def test_the_table_shapes_are_the_ones_the_kernels_need():
    shapes = {name: (blocks_cases.case(name)["a"].shape[1], blocks_cases.case(name)["a"].shape[0], blocks_cases.case(name)["m_eq"])
              for name in blocks_cases.BUILDERS}
    long = 2 * 524288 + 77
    assert shapes == {"dual_both_kinds": (300, 200, 60), "dual_inequalities_only": (300, 120, 0), "primal_forced": (300, 120, 0),
                      "primal_natural": (120, 300, 0), "all_equalities": (300, 100, 100), "one_slack": (257, 129, 128),
                      "one_equality": (257, 129, 1), "empty_columns_and_rows": (300, 200, 60), "open_box": (300, 200, 60),
                      "long_variables": (long, 40, 12), "long_rows": (30, long, 0),
                      "long_slacks_behind_equalities": (200, 524288 + 300 + 77, 300), "csrless": (3000, 4000, 300),
                      "scaled_equalities": (300, 200, 60), "step_limits": (600, 200, 200)}
    for name in blocks_cases.BUILDERS:
        assert blocks_cases.case(name)["a"].nnz <= 2_000_000
    base = blocks_cases.case("dual_both_kinds")
    bl, bu = base["b_lower"][60:], base["b_upper"][60:]
    assert np.sum(bl == bu) == 5 and 30 <= np.sum(bl == -np.inf) <= 65 and np.all(bl <= bu)
    empty = blocks_cases.case("empty_columns_and_rows")
    cols = empty["empty_cols"]
    assert np.all(np.diff(empty["a"].tocsc().indptr)[cols] == 0) and cols.size == 40 and np.sum(np.diff(empty["a"].indptr)[60:] == 0) >= 10
    assert np.sum((empty["c"][cols] != 0) & np.isfinite(empty["lb"][cols])) >= 10
    box = blocks_cases.case("open_box")
    assert 100 <= np.sum(np.isinf(box["lb"]) & np.isinf(box["ub"])) <= 200
    assert np.sum(np.diff(blocks_cases.case("long_variables")["a"].tocsc().indptr) > 0) < 500
    assert np.sum(np.diff(blocks_cases.case("csrless")["a"].tocsc().indptr) == 0) >= 50
    scaled = blocks_cases.case("scaled_equalities")
    assert np.allclose(scaled["a"][:3].toarray(), (np.array([[1.0], [10.0], [100.0]]) * base["a"][:3].toarray()))


def test_the_step_limit_case_needs_more_steps_than_its_largest_cap():
    case = blocks_cases.case("step_limits")
    a, m_eq = case["a"], case["m_eq"]
    cg = blocks_cpu.CgProjector(a, m_eq, case["b_upper"].copy(), tol=1e-13, max_steps=500)
    xs, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=1, x0=case["x0"], project=cg)
    print("conjugate-gradient steps of the first projection:", cg.steps)
    assert 25 < cg.steps < 500
    exact, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=1, x0=case["x0"])
    assert _rel(xs[0], exact[0]) < 1e-9
    # the error of the capped runs in the reference's arithmetic: the S-norm of the CG error never increases
    errs = []
    for cap in (3, 7, 10, 13, 25):
        capped, _ = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=1, x0=case["x0"],
                                           project=blocks_cpu.CgProjector(a, m_eq, case["b_upper"].copy(), max_steps=cap))
        errs.append(float(np.linalg.norm(capped[0] - exact[0])))
    assert all(hi >= lo * (1 - 1e-10) for hi, lo in zip(errs, errs[1:])) and errs[-1] < errs[0] and errs[-1] > 1e-6 * errs[0]


def test_the_fuzz_generator_keeps_four_fifths_of_its_draws_and_reaches_every_branch():
    lps, redraws = fuzz_projection.draws(fuzz_projection.TEST_CASES, fuzz_projection.TEST_SEED)
    print("redraws:", redraws, "of", len(lps) + redraws)
    for k, lp in enumerate(lps):
        print(k, fuzz_projection.describe(lp), f"condition {lp['projector'].condition:.3g}")
    assert len(lps) == fuzz_projection.TEST_CASES and 5 * redraws <= len(lps) + redraws
    assert all(lp["projector"].condition <= 1e6 and lp["projector"].lambda_min > 0 for lp in lps)
    assert {lp["solver"] for lp in lps} == {"blocks", "jacobi", "admm2"}
    assert {lp["min_nnz"] for lp in lps} == {"1", "100000000000"}
    assert {lp["forced"] for lp in lps} == {None, "0", "1"}
    assert any(lp["solver"] == "admm2" and lp["x0"] is not None for lp in lps) and any(lp["solver"] == "admm2" and lp["x0"] is None for lp in lps)
    assert any(lp["iterations"] == 1 for lp in lps) and any(lp["iterations"] > 1 for lp in lps)
    assert any(lp["a"].shape[0] > lp["a"].shape[1] for lp in lps) and any(lp["a"].shape[0] < lp["a"].shape[1] for lp in lps)
    assert any(lp["m_eq"] == 0 for lp in lps) and any(lp["m_eq"] == lp["a"].shape[0] for lp in lps)
    assert any(lp["projector"].primal and lp["a"].shape[0] < lp["a"].shape[1] for lp in lps)      # primal forced on m < n
    assert any(not lp["projector"].primal and lp["m_eq"] == 0 and lp["a"].shape[0] >= lp["a"].shape[1] for lp in lps)   # dual forced on m >= n
    again, _ = fuzz_projection.draws(fuzz_projection.TEST_CASES, fuzz_projection.TEST_SEED)
    assert all((x["a"] != y["a"]).nnz == 0 and x["solver"] == y["solver"] for x, y in zip(lps, again))
