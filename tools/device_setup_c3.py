"""The reference's entry points on BASELINE config 3 with ``setup="device"``, next to the repo API on the same LP.

The config-3 LP (random_lp_on_device: 1e6 variables x 2e6 rows at 1e-3, 2e9 stored entries) is generated on the device,
downloaded as a host scipy CSR (about 24 GB of host memory) and the device copy freed.  Then, alternating, in one process:
``SparseLP.solve(method="admm", xstep="auto")`` (the matrix-free ADMM at reuse level 0, device set-up) against ``DeviceADMM``
at level 0; ``SparseLP.solve(method="chambolle_pock_ppd")`` against ``DeviceCP(remove_fixed=True)``; ``lp_admm_cg(reuse=4, setup="device")``
against ``DeviceADMM`` at level 4 (the bench's).  The repo-API side regenerates the LP on the device, as bench.py does, and is
driven at the same report cadence (``--plot`` iterations: a report, the download of x, the multiplier half).

Per run: seconds from the call to the first report, steady-state iterations per second from the report timestamps (between the
second and the last report; for ``solve`` also with the time of its host-side curve bookkeeping -- ``max_constraint_violation``,
one scipy product per report -- taken out), and whether x after the last iteration equals the repo API's bit for bit.

    python tools/device_setup_c3.py OUT_DIR [--iters 150] [--plot 50]   ->  OUT_DIR/device_setup_c3.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pysparselp_amd import _lib  # noqa: E402
from pysparselp_amd.SparseLP import SparseLP  # noqa: E402
from pysparselp_amd.admm_cg import DeviceADMM, lp_admm_cg  # noqa: E402
from pysparselp_amd.problems import random_lp_on_device  # noqa: E402
from pysparselp_amd.scale import DeviceCP  # noqa: E402

N, M, DENSITY, SEED = 1_000_000, 2_000_000, 1e-3, 0


def steady(stamps):
    """Iterations per second between the second and the last report (the first iteration builds the product copies)."""
    (i0, t0), (i1, t1) = stamps[1], stamps[-1]
    return (i1 - i0) / (t1 - t0)


def host_lp():
    a, xf, c, lb, ub, b = random_lp_on_device(N, M, DENSITY, seed=SEED)
    t = time.perf_counter()
    host = a.download()
    a.close()
    _lib.check(_lib.lib().slp_trim())
    indptr = host.indptr.astype(np.int32) if host.nnz < 2 ** 31 - 1 else host.indptr
    host = scipy.sparse.csr_matrix((host.data, host.indices, indptr), shape=host.shape)
    return host, c, lb, ub, b, time.perf_counter() - t


def as_sparse_lp(a, c, lb, ub, b):
    lp = SparseLP()
    lp.nb_variables = c.size
    lp.costsvector, lp.lower_bounds, lp.upper_bounds = c, lb, ub
    lp.is_integer = np.zeros(c.size, dtype=bool)
    a.__dict__["blocks"] = [(0, a.shape[0] - 1)]
    lp.a_inequalities, lp.b_lower, lp.b_upper = a, None, b
    lp.a_equalities = scipy.sparse.csr_matrix((0, c.size))
    lp.b_equalities = np.zeros(0)
    return lp


def run_solve(lp, method, iters, plot):
    stamps, host_s = [], [0.0]
    real = lp.max_constraint_violation

    def timed(sol):
        t = time.perf_counter()
        v = real(sol)
        host_s[0] += time.perf_counter() - t
        return v

    lp.max_constraint_violation = timed
    marks = []
    t0 = time.perf_counter()
    kw = {"xstep": "auto"} if method == "admm" else {}
    x, _ = lp.solve(method=method, nb_iter=iters, nb_iter_plot=plot, setup="device",
                    plot_solution=lambda it, sol, is_active_variable=None: (stamps.append((it, time.perf_counter())),
                                                                             marks.append(host_s[0])), **kw)
    total = time.perf_counter() - t0
    del lp.max_constraint_violation
    (i0, t_a), (i1, t_b) = stamps[1], stamps[-1]
    return {"first_report_s": stamps[0][1] - t0, "it_per_s": steady(stamps),
            "it_per_s_without_host_curves": (i1 - i0) / ((t_b - t_a) - (marks[-1] - marks[1])),
            "host_curve_s": host_s[0], "total_s": total, "reports": len(stamps)}, x


def run_cg4(args_, iters, plot):
    stamps = []
    t0 = time.perf_counter()
    x = lp_admm_cg(*args_, nb_iter=iters, nb_iter_plot=plot, reuse=4, setup="device",
                   callback_func=lambda it, *rest: stamps.append((it, time.perf_counter())))
    return {"first_report_s": stamps[0][1] - t0, "it_per_s": steady(stamps), "total_s": time.perf_counter() - t0,
            "reports": len(stamps)}, x


def run_api(method, iters, plot, reuse=0):
    """The repo API the bench times: LP generated on the device, solver on it, driven at the solve loop's cadence."""
    t0 = time.perf_counter()
    a, xf, c, lb, ub, b = random_lp_on_device(N, M, DENSITY, seed=SEED)
    t_gen = time.perf_counter() - t0
    # (Chambolle-Pock: with the fixed variables removed, as SparseLP.solve does -- the generator fixes those whose round2(t) is 0)
    s = DeviceADMM(a, b, c, lb, ub, reuse=reuse) if method == "admm" else DeviceCP(a, b, c, lb, ub, remove_fixed=True)
    n = c.size
    halves = (s.xstep, s.multiplier_step) if method == "admm" else (s.primal_step, s.dual_step)
    last = iters + 1 if method == "admm" else iters   # lp_admm: nb_iter + 1 iterations (ADMM.py:143); CP: nb_max_iter
    stamps, i = [], 0
    while i < last:
        if i % plot == 0:
            halves[0]()
            s.report()
            s.x(n) if method == "admm" else s.x_reduced()
            stamps.append((i, time.perf_counter()))
            halves[1]()
            i += 1
        else:
            k = min(plot - i % plot, last - i)
            s.iterate(k)
            i += k
    # solve's x puts a fixed variable at -lb (SparseLP.py:1259,1288: full - shift), DeviceCP.x() at +lb
    x = s.x(n) if method == "admm" else np.where(s.free, s.x(), -s.shift)
    out = {"generate_s": t_gen, "first_report_s": stamps[0][1] - t0 - t_gen, "it_per_s": steady(stamps),
           "total_s": time.perf_counter() - t0, "reports": len(stamps)}
    s.close()
    a.close()
    _lib.check(_lib.lib().slp_trim())
    return out, x


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--iters", type=int, default=150)
    p.add_argument("--plot", type=int, default=50)
    args = p.parse_args()
    _lib.lib(0)
    a, c, lb, ub, b, t_down = host_lp()
    res = {"config": {"n": N, "m": M, "density": DENSITY, "nnz": int(a.nnz), "iters": args.iters, "nb_iter_plot": args.plot}}
    os.makedirs(args.out, exist_ok=True)

    def save(key, value):   # after every run: what was measured survives a later failure
        res[key] = value
        print(key, json.dumps(value), flush=True)
        with open(os.path.join(args.out, "device_setup_c3.json"), "w") as f:
            json.dump(res, f, indent=1)

    save("download_s", t_down)
    r, x_solve = run_solve(as_sparse_lp(a, c, lb, ub, b), "admm", args.iters, args.plot)
    save("solve_admm_level0", r)
    r, x_api = run_api("admm", args.iters, args.plot, reuse=0)
    save("DeviceADMM_level0", r)
    save("admm_level0_x_equal", bool(np.array_equal(x_solve, x_api)))
    save("admm_level0_x_max_rel_diff", float(np.max(np.abs(x_solve - x_api) / (1 + np.abs(x_api)))))

    r, x_solve = run_solve(as_sparse_lp(a, c, lb, ub, b), "chambolle_pock_ppd", args.iters, args.plot)
    save("solve_cp", r)
    r, x_api = run_api("chambolle_pock_ppd", args.iters, args.plot)
    save("DeviceCP", r)
    save("cp_fixed_variables", int(np.count_nonzero(lb == ub)))
    save("cp_x_equal", bool(np.array_equal(x_solve, x_api)))
    save("cp_x_max_rel_diff", float(np.max(np.abs(x_solve - x_api) / (1 + np.abs(x_api)))))

    r, x_cg = run_cg4((c, None, None, a, None, b, lb, ub), args.iters, args.plot)
    save("lp_admm_cg_level4", r)
    r, x_api = run_api("admm", args.iters, args.plot, reuse=4)
    save("DeviceADMM_level4", r)
    save("admm_level4_x_equal", bool(np.array_equal(x_cg, x_api)))
    save("admm_level4_x_max_rel_diff", float(np.max(np.abs(x_cg - x_api) / (1 + np.abs(x_api)))))


if __name__ == "__main__":
    main()
