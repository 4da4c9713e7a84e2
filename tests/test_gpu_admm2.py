"""lp_admm2 (reference ADMM.py:272-474) on the GPU: iterates against the reference's LU form (tests/golden/admm2.npz), the
reference's golden curves through SparseLP.solve(method="admm2"), its calling contract, and DeviceADMM2 over every product
format and set-up route."""
import copy
import json
import os

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from conftest import GOLDEN, Recorder, lp_from_golden, load_golden, solver_args

pytestmark = pytest.mark.gpu

CASES = {"sc50a": "lp_sc50a", "sc105": "lp_sc105", "potts8": "lp_potts8", "potts50": "lp_potts50", "random0": "lp_random0",
         "random1": "lp_random1", "random2": "lp_random2", "l1svm": "ka_l1svm", "sc105_pre": "lp_sc105"}


@pytest.mark.parametrize("case", list(CASES))
def test_gpu_admm2_iterates_match_the_reference_lu_form(case):
    from pysparselp_amd.ADMM import lp_admm2

    g = load_golden("admm2")
    ref = {int(i): (x, e) for i, x, e in zip(g[f"{case}_it"], g[f"{case}_x"], g[f"{case}_e1"])}
    rec = Recorder()
    x = lp_admm2(*solver_args(load_golden(CASES[case])), nb_iter=200, nb_iter_plot=1, callback_func=rec,
                 use_preconditioning=case.endswith("_pre"))
    assert rec.it == list(range(201))
    for it, (xr, er) in ref.items():
        assert np.max(np.abs(rec.x[it] - xr) / (1 + np.abs(xr))) < 1e-8, it
        np.testing.assert_allclose(rec.e1[it], er, rtol=1e-7)
        assert rec.e2[it] == rec.e1[it] and rec.veq[it] == 0 and rec.vineq[it] == 0
    assert np.array_equal(x.view(np.uint64), rec.x[-1].view(np.uint64))


@pytest.mark.parametrize("case,key,nb_iter,points", [("sc105", "netlib_curves_SC105.json", 5000, 11),
                                                     ("potts50", "test_pott_segmentation_curves.json", 2000, 5)])
def test_gpu_admm2_reference_golden_curves(case, key, nb_iter, points):
    """tests/test_netlib.py and tests/test_pott_segmentation.py of the reference, method admm2, through SparseLP.solve."""
    from pysparselp_amd.SparseLP import SparseLP

    d = load_golden("lp_" + case)
    lp = lp_from_golden(d, SparseLP)
    lp.solve(method="admm2", get_timing=True, nb_iter=nb_iter, max_time=None, ground_truth=d["gt"], ground_truth_indices=d["gt_idx"],
             plot_solution=None, nb_iter_plot=500)
    ref = np.array(json.load(open(os.path.join(GOLDEN, "ref_admm2_curves.json")))[key])
    got = np.array(lp.distance_to_ground_truth)
    assert got.size == points and lp.itrn_curve == list(range(0, nb_iter + 1, 500))
    np.testing.assert_almost_equal(got, ref[:points])


def test_gpu_admm2_contract():
    from pysparselp_amd.ADMM import lp_admm2
    from pysparselp_amd.SparseLP import SparseLP

    d = load_golden("lp_potts8")
    args = solver_args(d)
    rec = Recorder()
    lp_admm2(*args, nb_iter=20, nb_iter_plot=7, callback_func=rec)
    assert rec.it == [0, 7, 14]
    rec = Recorder()
    x = lp_admm2(*args, nb_iter=50, nb_iter_plot=10, callback_func=rec, max_time=1e-9)  # stops at the first report, before its callback
    assert rec.it == [] and x.shape == (d["c"].size,) and np.all(np.isfinite(x))
    with pytest.raises(UnboundLocalError):
        lp_admm2(args[0], args[1], args[2], None, None, None, args[6], args[7])
    lp = lp_from_golden(d, SparseLP)
    before = copy.deepcopy(lp)
    out = lp.solve(method="admm2", get_timing=True, nb_iter=20, nb_iter_plot=10)
    assert isinstance(out, tuple) and len(out) == 2 and out[0].shape == (d["c"].size,) and out[1] > 0
    assert lp.itrn_curve == [0, 10, 20]
    for name in ("costsvector", "lower_bounds", "upper_bounds", "b_equalities", "b_lower", "b_upper"):
        assert np.array_equal(getattr(lp, name), getattr(before, name)), name
    for name in ("a_equalities", "a_inequalities"):
        a, b = getattr(lp, name), getattr(before, name)
        assert a.shape == b.shape and (a != b).nnz == 0, name
    x = lp.solve(method="admm2", get_timing=False, nb_iter=20, nb_iter_plot=10)
    assert np.array_equal(x, out[0])


def _device_lp(m_eq, seed=5, m=4000):
    """The LP of tests/test_admm_blocks.py::test_gpu_row_block_solver_matches_oracle at density 0.003 (rows of ~9 entries: the CSR
    products stay in sequential order, bit-identical to the strip copies)."""
    from pysparselp_amd.problems import random_lp_on_device

    n, p = 3000, 0.003
    a, xf, c, lb, ub, b = random_lp_on_device(n, m, p, seed=seed)
    ax = a.matvec(xf)
    rng = np.random.RandomState(8)
    b = b.copy()
    b[:m_eq] = ax[:m_eq]
    bl = np.where(rng.rand(m) < 0.5, -np.inf, ax - rng.rand(m))
    return a, c, lb, ub, b, bl


def _admm2_lu(c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub, nb_iter, gamma=0.7, alpha=1.95):
    """The reference's loop (ADMM.py:320-474, x0 = 0, no preconditioning): one sparse LU of the KKT matrix."""
    n, mi = c.size, a_ineq.shape[0]
    blocks = [[a_ineq, -scipy.sparse.eye(mi)]] if a_eq is None else [[a_eq, None], [a_ineq, -scipy.sparse.eye(mi)]]
    a = scipy.sparse.bmat(blocks).tocsr()
    big_n = n + mi
    cc, lo, hi = np.concatenate((c, np.zeros(mi))), np.concatenate((lb, b_lower)), np.concatenate((ub, b_upper))
    b = np.concatenate((np.zeros(0) if a_eq is None else beq, np.zeros(mi)))
    lu = scipy.sparse.linalg.splu(scipy.sparse.bmat([[gamma * scipy.sparse.eye(big_n), a.T], [a, None]]).tocsc())
    x = np.zeros(big_n)
    xp, lam = np.clip(x, lo, hi), np.zeros(big_n)
    for _ in range(nb_iter + 1):
        x = alpha * lu.solve(np.concatenate((-cc + gamma * xp - lam, b)))[:big_n] + (1 - alpha) * xp
        xp = np.clip(x + lam / gamma, lo, hi)
        lam = lam + gamma * (x - xp)
    return x[:n]


@pytest.mark.parametrize("m_eq", [300, 0])  # dual form (A A^T + [0; I]) / all inequalities, m >= n: primal form (I + A^T A)
def test_gpu_device_admm2_formats(monkeypatch, m_eq):
    """DeviceADMM2 on strip copies and on CSR: the same bits, within 1e-8 of the LU form, and every x-step's projection solved to
    the CG bar.  (The bar is on the recurrence residual; the true residual, applied afresh, carries the recurrence's rounding:
    within 2 x of it.)"""
    from pysparselp_amd.scale import DeviceADMM2

    tol, max_steps = 1e-13, 500
    xs = {}
    for min_nnz in ("1", "100000000000"):   # strip kernels / CSR kernels
        monkeypatch.setenv("SLP_STRIP_MIN_NNZ", min_nnz)
        a, c, lb, ub, b, bl = _device_lp(m_eq)
        assert (a.spmv_kernel(False) == 0) == (min_nnz != "1")
        if min_nnz == "1":
            s = a.download()
        sol = DeviceADMM2(a, b, c, lb, ub, m_eq=m_eq, b_lower=bl, cg_tol=tol, cg_max_steps=max_steps)
        steps = 0
        for it in range(30):
            sol.iterate(1)
            now = sol.cg_steps()
            res, rhs = sol.projection_residual()
            if now - steps < max_steps:
                assert res <= 2 * tol * rhs, (it, res, rhs)
            steps = now
        assert 30 < steps < 30 * max_steps
        xs[min_nnz] = sol.x()
        sol.close()
        a.close()
    assert np.array_equal(xs["1"].view(np.uint64), xs["100000000000"].view(np.uint64))
    xo = _admm2_lu(c, s[:m_eq] if m_eq else None, b[:m_eq] if m_eq else None, s[m_eq:], bl[m_eq:], b[m_eq:], lb, ub, nb_iter=29)
    assert np.max(np.abs(xs["1"] - xo) / (1 + np.abs(xo))) < 1e-8


def test_gpu_admm2_routes_are_bit_identical(monkeypatch):
    """lp_admm2 on the downloaded host CSR -- uploaded whole, or in row chunks -- and DeviceADMM2 on the device matrix; two runs
    of the first."""
    from pysparselp_amd import device
    from pysparselp_amd.ADMM import lp_admm2
    from pysparselp_amd.scale import DeviceADMM2

    # a chunk of a chunked matrix lives as its strip copies only, and a chunk's copy of its transpose needs >= 3 entries per
    # column: twice the rows, and 1200 equality rows (their own chunk)
    monkeypatch.setenv("SLP_STRIP_MIN_NNZ", "1")
    m_eq = 1200
    a, c, lb, ub, b, bl = _device_lp(m_eq, seed=6, m=8000)
    s = a.download()
    args = (c, s[:m_eq], b[:m_eq], s[m_eq:], bl[m_eq:], b[m_eq:], lb, ub)
    runs = [lp_admm2(*args, nb_iter=29, nb_iter_plot=10) for _ in range(2)]
    chunks = []
    append = device.ChunkedDeviceMatrix.append
    monkeypatch.setattr(device.ChunkedDeviceMatrix, "append", lambda self, chunk: (chunks.append(chunk.shape), append(self, chunk))[1])
    monkeypatch.setenv("SLP_SETUP_CHUNK_ENTRIES", str(s.nnz // 5))
    runs.append(lp_admm2(*args, nb_iter=29, nb_iter_plot=10))
    assert len(chunks) >= 3
    monkeypatch.delenv("SLP_SETUP_CHUNK_ENTRIES")
    sol = DeviceADMM2(a, b, c, lb, ub, m_eq=m_eq, b_lower=bl)
    sol.iterate(30)
    runs.append(sol.x())
    sol.close()
    a.close()
    for x in runs[1:]:
        assert np.array_equal(x.view(np.uint64), runs[0].view(np.uint64))
