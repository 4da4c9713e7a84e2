"""The matrix-free projection of csrc/slp_blocks.hip (DeviceBlocks, DeviceADMM2) at the edges of its kernels, against the exact
reference of tests/blocks_cpu.py on the LPs of tests/blocks_cases.py -- each the smallest shape at which its path exists:

  dual_both_kinds                dual form A A^T + [0; I] with equality, two-sided, one-sided and fixed (b_lower = b_upper) rows
  dual_inequalities_only         m < n, m_eq = 0: A A^T + I as the natural form
  primal_forced                  the same LP with SLP_BLOCKS_PRIMAL=1: I + A^T A on m < n
  primal_natural                 m >= n, m_eq = 0
  all_equalities                 no slack launch, gs = 0, energy partial sums of the variables alone
  one_slack / one_equality       the loops that start at + m_eq over one element / from row 1; sizes off every multiple of 64 and 256
  empty_columns_and_rows         used[j] = 0 / copies = 0 in the consensus and the energy; inequality rows without entries
  open_box                       lb = -inf, ub = +inf on half the variables
  long_variables                 n = 2 x 524288 + 77: three trips of every grid-stride loop over the variables, more than
                                 1024 x 256 elements in k_blk_dot and k_a2_x; most columns unused
  long_rows                      m = 2 x 524288 + 77, primal form: three trips of the slack loops from offset 0
  long_slacks_behind_equalities  m - m_eq above one grid behind 300 equality rows (dual form; conjugate-gradient reference)
  csrless                        the CSR released after both copies exist: column use from the product (|A|^0)^T 1

Every case runs on strip copies and on the CSR kernels (SLP_STRIP_MIN_NNZ).  (a) After ONE iteration from zero multipliers the
iterate is alpha P(v0) + (1 - alpha) xp0 -- DeviceADMM2 from a random x0 projects an arbitrary point -- and must lie within
``blocks_cpu.projection_bound`` of the reference, a bound formed from the reference's own matrices; the projection's true residual
must meet the bar 2 tol |rhs|.  (b) Eight iterations against the restated loops at the suite's 1e-8, the energy of every iteration
at rtol 1e-7, and a second run bit for bit.  (c) the same with the Jacobi preconditioner; (d) step limits."""
import numpy as np
import pytest

import blocks_cases
import blocks_cpu
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 1e-13
FORMATS = ["1", "100000000000"]   # SLP_STRIP_MIN_NNZ: strip copies / CSR kernels
ITERATIONS = 8
_REFERENCE = {}


def _reference(name, solver):
    """``(x per iteration, energy per iteration, Projection of the first iteration)``, computed once."""
    key = (name, solver)
    if key not in _REFERENCE:
        case = blocks_cases.case(name)
        a, m_eq = case["a"], case["m_eq"]
        b = np.concatenate((case["b_upper"][:m_eq], np.zeros(a.shape[0] - m_eq)))
        proj = blocks_cpu.ExactProjector(a, m_eq, b, blocks_cpu.device_primal(a.shape[0], a.shape[1], m_eq, case["forced"]))
        seen = []

        def project(v, vs):
            seen.append(proj.project(v, vs))
            return seen[-1].x, seen[-1].s

        if solver == "admm2":
            xs, es = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=ITERATIONS, x0=case["x0"], project=project)
        else:
            xs, es = blocks_cpu.blocks_exact(*blocks_cases.lp_args(case), nb_iter=ITERATIONS, project=project)
        _REFERENCE[key] = (xs, es, seen[0], proj)
    return _REFERENCE[key]


def _environment(monkeypatch, case, min_nnz):
    monkeypatch.setenv("SLP_STRIP_MIN_NNZ", min_nnz)
    if case["forced"] is None:
        monkeypatch.delenv("SLP_BLOCKS_PRIMAL", raising=False)
    else:
        monkeypatch.setenv("SLP_BLOCKS_PRIMAL", case["forced"])


def _solver(solver, a, case, **kw):
    from pysparselp_amd.scale import DeviceADMM2, DeviceBlocks

    if solver == "admm2":
        return DeviceADMM2(a, case["b_upper"], case["c"], case["lb"], case["ub"], m_eq=case["m_eq"], b_lower=case["b_lower"],
                           x0=kw.pop("x0", case["x0"]), cg_tol=TOL, **kw)
    return DeviceBlocks(a, case["b_upper"], case["c"], case["lb"], case["ub"], m_eq=case["m_eq"], b_lower=case["b_lower"], cg_tol=TOL,
                        jacobi=solver == "jacobi", **kw)


def _rel(x, ref):
    return float(np.max(np.abs(x - ref) / (1 + np.abs(ref))))


def _one_projection_then_the_trajectory(monkeypatch, name, solver, min_nnz):
    from pysparselp_amd.device import DeviceMatrix

    case = blocks_cases.case(name)
    xs, es, first, proj = _reference(name, "admm2" if solver == "admm2" else "blocks")
    _environment(monkeypatch, case, min_nnz)
    a = DeviceMatrix.from_csr(case["a"])
    sol = _solver(solver, a, case)
    print(f"{name} {solver} SLP_STRIP_MIN_NNZ={min_nnz}: kernels {a.spmv_kernel(False)} / {a.spmv_kernel(True)}, "
          f"primal {proj.primal}, condition {proj.condition:.3g}")
    atol = 0.0 if solver == "admm2" else 1e-7   # (the bars of tests/test_gpu_admm2.py / tests/test_admm_blocks.py)
    try:
        # (a) one projection
        sol.iterate(1)
        x = sol.x()
        bound = blocks_cpu.projection_bound(first, case["a"], TOL)
        err = float(np.linalg.norm(x - xs[0]))
        res, rhs = sol.projection_residual()
        print(f"  one projection: error {err:.3g}, bound {bound:.3g}, error / bound {err / bound:.3g}; residual {res:.3g}, "
              f"2 tol |rhs| {2 * TOL * rhs:.3g}; conjugate-gradient steps {sol.cg_steps()}")
        assert err <= bound
        assert res <= 2 * TOL * rhs
        assert abs(rhs - first.rhs_norm) <= 1e-9 * first.rhs_norm
        np.testing.assert_allclose(sol.report()[0], es[0], rtol=1e-7, atol=atol)
        # (b) the trajectory
        for it in range(1, ITERATIONS):
            sol.iterate(1)
            rel = _rel(sol.x(), xs[it])
            print(f"  iteration {it}: {rel:.3g}")
            assert rel < 1e-8, it
            np.testing.assert_allclose(sol.report()[0], es[it], rtol=1e-7, atol=atol, err_msg=f"energy of iteration {it}")
        x = sol.x()
        steps = sol.cg_steps()
    finally:
        sol.close()
    again = _solver(solver, a, case)
    try:
        again.iterate(ITERATIONS)
        assert np.array_equal(again.x().view(np.uint64), x.view(np.uint64)) and again.cg_steps() == steps
    finally:
        again.close()
        a.close()


@pytest.mark.parametrize("min_nnz", FORMATS)
@pytest.mark.parametrize("name", blocks_cases.TABLE)
def test_admm2_one_projection_and_trajectory(monkeypatch, name, min_nnz):
    _one_projection_then_the_trajectory(monkeypatch, name, "admm2", min_nnz)


@pytest.mark.parametrize("min_nnz", FORMATS)
@pytest.mark.parametrize("name", blocks_cases.TABLE)
def test_blocks_one_projection_and_trajectory(monkeypatch, name, min_nnz):
    _one_projection_then_the_trajectory(monkeypatch, name, "blocks", min_nnz)


@pytest.mark.parametrize("min_nnz", FORMATS)
@pytest.mark.parametrize("name", blocks_cases.JACOBI)
def test_blocks_jacobi_one_projection_and_trajectory(monkeypatch, name, min_nnz):
    """(c) Against the exact reference, not against the plain run.  ``scaled_equalities``: the equality rows scaled by 1, 10, 100 in
    turn, so diag(A A^T) is far from constant and a ``+ 1`` on the wrong side of m_eq changes the preconditioner."""
    _one_projection_then_the_trajectory(monkeypatch, name, "jacobi", min_nnz)


@pytest.mark.parametrize("min_nnz", FORMATS)
def test_admm2_long_slack_range_behind_equality_rows(monkeypatch, min_nnz):
    """(b') m - m_eq = 524288 + 77 slacks behind 300 equality rows: the slack loops start at + m_eq and take two trips.  The dual
    system has m rows and the primal form does not exist with equality rows, so this is the ONLY case without the exact
    reference: three iterations from x0 against ``admm2_matrix_free`` generalised to a starting point
    (``blocks_cpu.CgProjector`` in ``admm2_exact``), at 1e-8.  300 equality rows over 200 variables are rank deficient, the system
    singular but consistent: conjugate gradients converge on it in about 500 steps per projection, so both sides run with a step
    limit of 2000 (at the default 500 neither side has converged and they differ by 2e-3)."""
    from pysparselp_amd.device import DeviceMatrix

    case = blocks_cases.case("long_slacks_behind_equalities")
    a_host, m_eq = case["a"], case["m_eq"]
    if "long_slacks" not in _REFERENCE:
        b = np.concatenate((case["b_upper"][:m_eq], np.zeros(a_host.shape[0] - m_eq)))
        _REFERENCE["long_slacks"] = blocks_cpu.admm2_exact(*blocks_cases.lp_args(case), nb_iter=3, x0=case["x0"],
                                                           project=blocks_cpu.CgProjector(a_host, m_eq, b, tol=TOL, max_steps=2000))
    xs, es = _REFERENCE["long_slacks"]
    _environment(monkeypatch, case, min_nnz)
    a = DeviceMatrix.from_csr(a_host)
    sol = _solver("admm2", a, case, cg_max_steps=2000)
    print(f"kernels {a.spmv_kernel(False)} / {a.spmv_kernel(True)}")
    try:
        before = 0
        for it in range(3):
            sol.iterate(1)
            rel = _rel(sol.x(), xs[it])
            print(f"  iteration {it}: {rel:.3g}, conjugate-gradient steps {sol.cg_steps() - before}")
            assert sol.cg_steps() - before < 2000, it   # (converged, not stopped at the limit)
            before = sol.cg_steps()
            assert rel < 1e-8, it
            np.testing.assert_allclose(sol.report()[0], es[it], rtol=1e-7)
    finally:
        sol.close()
        a.close()


def test_solvers_set_up_after_the_csr_entries_are_released(monkeypatch):
    """50 columns without entries and no CSR to read that from: ``k_rb_used_counts``.  Five iterations of both solvers against the
    sparse-LU loops the suite already trusts (the dense side is too large for the exact reference)."""
    from pysparselp_amd import _lib
    from pysparselp_amd.device import DeviceMatrix
    from test_gpu_admm2 import _admm2_lu

    case = blocks_cases.case("csrless")
    monkeypatch.setenv("SLP_STRIP_MIN_NNZ", "1")
    monkeypatch.delenv("SLP_BLOCKS_PRIMAL", raising=False)
    m = case["a"].shape[0]
    args = blocks_cases.solver_args_of(case)
    x_blocks = oracle.lp_admm_block_decomposition(*args, nb_iter=4, nb_iter_plot=10 ** 9, blocks_eq=[(0, m - 1)], blocks_ineq=[])
    x_admm2 = _admm2_lu(*args, nb_iter=4)
    a = DeviceMatrix.from_csr(case["a"])
    early = _solver("blocks", a, case)   # builds both copies
    print(f"kernels {a.spmv_kernel(False)} / {a.spmv_kernel(True)}")
    a.release_csr()
    with pytest.raises(_lib.SlpError, match="released"):
        a.download()
    out = {}
    for solver in ("blocks", "admm2"):
        sol = _solver(solver, a, case, **({"x0": None} if solver == "admm2" else {}))
        sol.iterate(5)
        out[solver] = sol.x()
        res, rhs = sol.projection_residual()
        assert res <= 2 * TOL * rhs
        sol.close()
    early.iterate(5)
    assert np.array_equal(early.x(), out["blocks"])   # column use from the transposed CSR == from the counts
    early.close()
    a.close()
    cols = case["empty_cols"]
    print("blocks", _rel(out["blocks"], x_blocks), "admm2", _rel(out["admm2"], x_admm2))
    assert _rel(out["blocks"], x_blocks) < 1e-8 and _rel(out["admm2"], x_admm2) < 1e-8
    assert np.any(out["blocks"][cols] != 0.0)


CAPS = (3, 7, 10, 13, 25)


@pytest.mark.parametrize("min_nnz", FORMATS)
def test_step_limits_off_the_check_interval(monkeypatch, min_nnz):
    """(d) n = 600, m_eq = m = 200 needs 224 steps to 1e-13 (tests/test_blocks_cpu_host.py).  A cap that is no multiple of the check
    interval (10) ends a run on a shorter chunk than the captured graph's: the step count is the cap exactly, and with all rows
    equalities from nu = 0 the error |x_k - x*|_2 is the S-norm of the conjugate-gradient error, which never increases."""
    from pysparselp_amd.device import DeviceMatrix

    case = blocks_cases.case("step_limits")
    xs, _, first, _ = _reference("step_limits", "admm2")
    _environment(monkeypatch, case, min_nnz)
    a = DeviceMatrix.from_csr(case["a"])
    try:
        errs = {}
        for cap in CAPS:
            sol = _solver("admm2", a, case, cg_max_steps=cap)
            sol.iterate(1)
            assert sol.cg_steps() == cap
            errs[cap] = float(np.linalg.norm(sol.x() - xs[0]))
            if cap == 25:
                deltas, before = [], sol.cg_steps()
                for _ in range(3):
                    sol.iterate(1)
                    deltas.append(sol.cg_steps() - before)
                    before = sol.cg_steps()
                print("steps per iteration at cap 25:", [25] + deltas)
                assert set(deltas) <= {0, 10, 20, 25}
            sol.close()
        print("errors:", errs)
        for lo, hi in zip(CAPS, CAPS[1:]):
            assert errs[lo] >= errs[hi] * (1 - 1e-10), (lo, hi)
        assert errs[25] < errs[3]
        sol = _solver("admm2", a, case, cg_max_steps=500)
        sol.iterate(1)
        steps = sol.cg_steps()
        res, rhs = sol.projection_residual()
        print("steps at cap 500:", steps, "residual", res, "bar", 2 * TOL * rhs)
        assert steps % 10 == 0 and 25 < steps < 500
        assert res <= 2 * TOL * rhs
        assert float(np.linalg.norm(sol.x() - xs[0])) <= blocks_cpu.projection_bound(first, case["a"], TOL)
        sol.close()
    finally:
        a.close()
