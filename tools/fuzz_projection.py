"""Randomised cross-check of the matrix-free projection solvers (csrc/slp_blocks.hip: DeviceBlocks, with and without the Jacobi
preconditioner, and DeviceADMM2) against the exact reference of tests/blocks_cpu.py: n, m in [1, 400] with either side the long
one, m_eq in {0, 1, m // 3, m - 1, m} (as far as the equality rows can have full rank: at most three quarters of n), rows of 1 to 12
entries, random shares of one-sided, fixed and unbounded rows and of variables without bounds, a starting point or none, the form of
the projection forced or not (SLP_BLOCKS_PRIMAL), strip copies or CSR kernels (SLP_STRIP_MIN_NNZ), 1 to 6 iterations.  A draw of one
iteration is checked against the error bound of one projection (``blocks_cpu.projection_bound``) and the residual bar, a longer
one iterate by iterate at 1e-8 (energies at rtol 1e-7).  A draw whose system has a condition number above 1e6, or an equality row
without entries, is drawn again (singular systems are out of scope: the reference project's LU cannot do them either); the run
fails if that happens to more than a fifth of the draws.
python tools/fuzz_projection.py [--cases 24] [--seed 0]"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

TEST_CASES, TEST_SEED = 24, 20
MAX_CONDITION = 1e6
TOL = 1e-13


def draw(rng):
    """One LP and how to run it; no check of its conditioning."""
    import blocks_cases

    n, m = int(rng.randint(1, 401)), int(rng.randint(1, 401))
    options = sorted({v for v in (0, 1, m // 3, m - 1, m) if 0 <= v <= 0.75 * n})
    m_eq = int(rng.choice(options))
    a = blocks_cases.sparse_rows(rng, m, n, 1, min(12, n))
    lp = blocks_cases.lp_around(rng, a, m_eq, no_lower=float(rng.choice([0.0, 0.3, 1.0])), fixed=int(rng.choice([0, 1, 5])),
                                open_box=float(rng.choice([0.0, 0.2, 1.0])))
    no_upper = rng.rand(m) < float(rng.choice([0.0, 0.2]))
    no_upper[:m_eq] = False
    no_upper &= lp["b_lower"] != lp["b_upper"]
    lp["b_upper"] = np.where(no_upper, np.inf, lp["b_upper"])
    lp["solver"] = str(rng.choice(["blocks", "jacobi", "admm2"]))
    if rng.rand() < 0.5:
        lp["x0"] = None
    lp["forced"] = rng.choice([None, "0", "1"] if m_eq == 0 else [None, "0"])
    lp["min_nnz"] = str(rng.choice(["1", "100000000000"]))
    lp["iterations"] = int(rng.randint(1, 7))
    return lp


def draws(cases, seed):
    """``cases`` draws whose reference system is regular (condition <= 1e6, no empty equality row), each with its
    ``blocks_cpu.ExactProjector`` under ``"projector"``, and the number of draws thrown away."""
    import blocks_cpu

    rng = np.random.RandomState(seed)
    out, redraws = [], 0
    while len(out) < cases:
        lp = draw(rng)
        a, m_eq = lp["a"], lp["m_eq"]
        b = np.concatenate((lp["b_upper"][:m_eq], np.zeros(a.shape[0] - m_eq)))
        primal = blocks_cpu.device_primal(a.shape[0], a.shape[1], m_eq, lp["forced"])
        proj = blocks_cpu.ExactProjector(a, m_eq, b, primal)
        if np.any(np.diff(a.indptr)[:m_eq] == 0) or not proj.condition <= MAX_CONDITION:
            redraws += 1
            continue
        lp["projector"] = proj
        out.append(lp)
    return out, redraws


def check_one_projection(sol, x, ref_x, proj, first, a, what):
    """Part (a): the iterate after one iteration inside the reference's bound, the projection's residual at the bar."""
    import blocks_cpu

    bound = blocks_cpu.projection_bound(first, a, TOL)
    err = float(np.linalg.norm(x - ref_x))
    res, rhs = sol.projection_residual()
    print(f"{what}: error / bound = {err / bound:.3g} (bound {bound:.3g}), residual / (2 tol rhs) = {res / (2 * TOL * rhs) if rhs else 0.0:.3g}, "
          f"condition {proj.condition:.3g}", flush=True)
    assert err <= bound, f"{what}: |x - x_ref| = {err} above the bound {bound}"
    assert res <= 2 * TOL * rhs, f"{what}: projection residual {res} above 2 tol |rhs| = {2 * TOL * rhs}"
    assert abs(rhs - first.rhs_norm) <= 1e-9 * first.rhs_norm, f"{what}: |rhs| {rhs} is not the reference's {first.rhs_norm}"
    return err / bound


def run_draw(lp, what="draw"):
    """Runs one draw on the device and checks it; returns the error / bound ratio of a one-iteration draw, else None."""
    import blocks_cases
    import blocks_cpu
    from pysparselp_amd.device import DeviceMatrix
    from pysparselp_amd.scale import DeviceADMM2, DeviceBlocks

    proj, its = lp["projector"], lp["iterations"]
    firsts = []

    def project(v, vs):
        p = proj.project(v, vs)
        firsts.append(p)
        return p.x, p.s

    args = blocks_cases.lp_args(lp)
    if lp["solver"] == "admm2":
        ref_x, ref_e = blocks_cpu.admm2_exact(*args, nb_iter=its, x0=lp["x0"], project=project)
    else:
        ref_x, ref_e = blocks_cpu.blocks_exact(*args, nb_iter=its, project=project)
    os.environ["SLP_STRIP_MIN_NNZ"] = lp["min_nnz"]
    if lp["forced"] is None:
        os.environ.pop("SLP_BLOCKS_PRIMAL", None)
    else:
        os.environ["SLP_BLOCKS_PRIMAL"] = lp["forced"]
    a = DeviceMatrix.from_csr(lp["a"])
    try:
        if lp["solver"] == "admm2":
            sol = DeviceADMM2(a, lp["b_upper"], lp["c"], lp["lb"], lp["ub"], m_eq=lp["m_eq"], b_lower=lp["b_lower"], x0=lp["x0"], cg_tol=TOL)
        else:
            sol = DeviceBlocks(a, lp["b_upper"], lp["c"], lp["lb"], lp["ub"], m_eq=lp["m_eq"], b_lower=lp["b_lower"], cg_tol=TOL,
                               jacobi=lp["solver"] == "jacobi")
        print(f"{what}: kernels {a.spmv_kernel(False)} / {a.spmv_kernel(True)}", flush=True)
        ratio = None
        try:
            for it in range(its):
                sol.iterate(1)
                x, energy = sol.x(), float(sol.report()[0])
                if its == 1:
                    ratio = check_one_projection(sol, x, ref_x[0], proj, firsts[0], lp["a"], what)
                else:
                    err = float(np.max(np.abs(x - ref_x[it]) / (1 + np.abs(ref_x[it]))))
                    assert err < 1e-8, f"{what}: iteration {it}: {err}"
                np.testing.assert_allclose(energy, ref_e[it], rtol=1e-7, err_msg=f"{what}: energy of iteration {it}")
        finally:
            sol.close()
    finally:
        a.close()
    return ratio


def describe(lp):
    m, n = lp["a"].shape
    return (f"{lp['solver']} n={n} m={m} m_eq={lp['m_eq']} nnz={lp['a'].nnz} x0={'yes' if lp['x0'] is not None else 'no'} "
            f"forced={lp['forced']} min_nnz={lp['min_nnz']} iterations={lp['iterations']}")


def run(cases, seed, verbose=False):
    keys = ("SLP_STRIP_MIN_NNZ", "SLP_BLOCKS_PRIMAL")
    saved = {k: os.environ.get(k) for k in keys}
    lps, redraws = draws(cases, seed)
    counts = {"cases": 0, "redraws": redraws, "one_projection": 0, "worst_ratio": 0.0}
    try:
        for k, lp in enumerate(lps):
            what = f"seed {seed} case {k} ({describe(lp)})"
            if verbose:
                print(what, flush=True)
            ratio = run_draw(lp, what)
            counts["cases"] += 1
            if ratio is not None:
                counts["one_projection"] += 1
                counts["worst_ratio"] = max(counts["worst_ratio"], ratio)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert 5 * redraws <= cases + redraws, f"{redraws} of {cases + redraws} draws were thrown away: more than a fifth"
    return counts


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", type=int, default=TEST_CASES)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--verbose", action="store_true")
    args = p.parse_args()
    print("ok:", run(args.cases, args.seed, args.verbose))


if __name__ == "__main__":
    main()
