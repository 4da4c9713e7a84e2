"""lp_admm2 (ADMM with exact equality projections, DeviceADMM2) at scale: the synthetic LP of bench.py generated on the
device (same generator and seed), a warm-up, then timed iterations with product timing on around them.

    python tools/bench_admm2.py OUTDIR [--config c3] [--iters N] [--warmup W]

Writes one JSON line (stdout and OUTDIR/admm2_<config>.json): iterations per second, CG steps per iteration, ms per CG step,
the share of the timed region spent in the products (slp_product_timing), set-up seconds and the objective.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--config", default="c3")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    import bench
    from pysparselp_amd import _lib
    from pysparselp_amd.problems import random_lp_on_device
    from pysparselp_amd.scale import DeviceADMM2

    n, m, density = bench.CONFIGS[args.config]
    lib = _lib.lib()
    t0 = time.perf_counter()
    a, xf, c, lb, ub, b = random_lp_on_device(n, m, density, seed=args.seed)
    _lib.check(lib.slp_synchronize())
    t_generate = time.perf_counter() - t0
    t1 = time.perf_counter()
    solver = DeviceADMM2(a, b, c, lb, ub)
    _lib.check(lib.slp_synchronize())
    t_setup = time.perf_counter() - t1
    solver.iterate(args.warmup)
    _lib.check(lib.slp_synchronize())
    cg0 = solver.cg_steps()
    _lib.check(lib.slp_product_timing(1))
    t0 = time.perf_counter()
    solver.iterate(args.iters)
    _lib.check(lib.slp_synchronize())
    dt = time.perf_counter() - t0
    _lib.check(lib.slp_product_timing(0))
    prod = np.zeros(3)
    _lib.check(lib.slp_product_timing_read(_lib.ptr(prod)))   # products, sum of their durations (ms), the longest (ms)
    steps = solver.cg_steps() - cg0
    energy = float(solver.report()[0])
    out = {
        "method": "admm2", "config": args.config, "n": n, "m": m, "density": density, "nnz": int(a.nnz),
        "projection": "primal (I + A^T A)" if m >= n else "dual (A A^T + I)",
        "kernels": [a.spmv_kernel(False), a.spmv_kernel(True)],
        "warmup": args.warmup, "iterations": args.iters, "seconds": dt,
        "it_per_s": args.iters / dt,
        "cg_steps_per_iteration": steps / args.iters,
        "ms_per_cg_step": 1e3 * dt / max(steps, 1),
        "products": int(prod[0]), "products_ms": float(prod[1]), "longest_product_ms": float(prod[2]),
        "products_share_of_timed_region": float(prod[1]) / (1e3 * dt),
        "generate_seconds": t_generate, "setup_seconds": t_setup,
        "objective": solver.objective(), "energy": energy,
        "feasible_x_objective": float(np.dot(c, xf)),
    }
    solver.close()
    a.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, f"admm2_{args.config}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
