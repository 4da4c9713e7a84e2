"""Dual gradient ascent (DeviceDGA, csrc/slp_dga.hip) measured: the synthetic LP of bench.py at a BASELINE config (generated on the
device, same generator and seed) or the Potts n x n LP, a warm-up, then timed iterations with the stage timer on around them.

    python tools/bench_dga.py OUTDIR [--config c3 | --potts 256] [--iters N] [--warmup W] [--path auto|fused|general]

Writes one JSON line (stdout and OUTDIR/dga_<config>.json | dga_potts<n>.json, with _<path> appended when a path is forced):
iterations per second (host clock around the timed iterations, ended by a device synchronise), the time per iteration of the products, the sort, the scans, the fused
search and the rest (HIP event pairs at the stage boundaries, read after the timed region), the share of an iteration spent
outside the products, and the comparison partner: tests/dga_cpu.py in the reference's order on one core -- at full size for
Potts, on the first rows of the same LP (all n columns) scaled by the row ratio for a config (as bench.py's cpu_baseline;
the search over the n breakpoints does not shrink with the rows, so the scaled figure flatters the CPU a little).
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def cpu_rate(args_cpu, iters):
    """Iterations per second of dga_cpu(order="reference"): whole iterations between its line searches' time stamps."""
    from dga_cpu import dga_cpu

    stamps = []
    t0 = time.perf_counter()
    dga_cpu(*args_cpu, nb_max_iter=iters, order="reference", on_search=lambda it, *rest: stamps.append((it, time.perf_counter())))
    total = time.perf_counter() - t0
    first = {}
    for it, t in stamps:
        first.setdefault(it, t)
    its = sorted(first)
    if len(its) >= 3:
        return (its[-1] - its[1]) / (first[its[-1]] - first[its[1]]), total
    return iters / total, total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--config", default="c3")
    p.add_argument("--potts", type=int, default=0)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--path", default="auto")
    p.add_argument("--cpu-iters", type=int, default=4)
    p.add_argument("--cpu-sample-entries", type=float, default=1.0e8)
    args = p.parse_args()
    import scipy.sparse

    import bench
    from pysparselp_amd import _lib
    from pysparselp_amd.DualGradientAscent import DeviceDGA
    from pysparselp_amd.device import DeviceMatrix
    from pysparselp_amd.problems import potts_lp, random_lp_on_device

    lib = _lib.lib()
    t0 = time.perf_counter()
    if args.potts:
        name = f"potts{args.potts}"
        lp = potts_lp(args.potts)[0]
        assert lp.b_lower is None or np.max(lp.b_lower) == -np.inf
        a_eq, a_ineq = lp.a_equalities, lp.a_inequalities
        m_eq = a_eq.shape[0]
        c, lb, ub = lp.costsvector, lp.lower_bounds, lp.upper_bounds
        b = np.concatenate((lp.b_equalities if m_eq else np.zeros(0), lp.b_upper))
        a = DeviceMatrix.from_blocks(a_eq if m_eq else None, a_ineq, c.size)
        m, n, density = a.shape[0], a.shape[1], None
        cpu_args = (c, a_eq, lp.b_equalities, a_ineq, lp.b_upper, lb, ub)
        scale, sample_rows = 1.0, m
    else:
        name = args.config
        n, m, density = bench.CONFIGS[args.config]
        a, xf, c, lb, ub, b = random_lp_on_device(n, m, density, seed=args.seed)
        m_eq = 0
        # the CPU's sample: the first rows of the same LP, all n columns
        sample_rows = max(1, min(m, int(args.cpu_sample_entries / max(n * density, 1.0))))
        sa = DeviceMatrix.random(sample_rows, n, density, args.seed)
        s = sa.download()
        sa.close()
        cpu_args = (c, scipy.sparse.csr_matrix((0, n)), np.zeros(0), s, b[:sample_rows], lb, ub)
        scale = sample_rows / m
    _lib.check(lib.slp_synchronize())
    t_generate = time.perf_counter() - t0
    rs = np.random.RandomState(0)
    y0 = np.concatenate((-rs.rand(m_eq), np.abs(rs.rand(m - m_eq))))
    t1 = time.perf_counter()
    solver = DeviceDGA(a, b, c, lb, ub, y0, m_eq=m_eq, draws=rs.random_sample, path=args.path)
    _lib.check(lib.slp_synchronize())
    t_setup = time.perf_counter() - t1
    e0 = solver.report()[0]
    solver.iterate(args.warmup)
    _lib.check(lib.slp_synchronize())
    solver.status()
    solver.push_random(rs.random_sample(2 * args.iters))
    solver.timing(True)
    t0 = time.perf_counter()
    solver.iterate(args.iters, refill=False)
    _lib.check(lib.slp_synchronize())
    dt = time.perf_counter() - t0
    solver.timing(False)
    stages = solver.timing_read()
    flags, draws, _, iters_done = solver.status()
    assert iters_done == args.warmup + args.iters
    energy, max_violation, sum_violation = solver.report()
    per_iter = {k: v / args.iters for k, v in stages.items()}
    events_ms = sum(per_iter.values())
    cpu_sample_rate, cpu_seconds = cpu_rate(cpu_args, args.cpu_iters)
    out = {
        "method": "dual_gradient_ascent", "workload": name, "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
        "n": int(n), "m": int(m), "m_eq": int(m_eq), "density": density, "nnz": int(a.nnz),
        "kernels": [a.spmv_kernel(False), a.spmv_kernel(True)], "search_path": solver.path(),
        "products_per_iteration": 5 if 0 < m_eq < m else 3,
        "warmup": args.warmup, "iterations": args.iters, "seconds": dt, "it_per_s": args.iters / dt,
        "ms_per_iteration_host_clock": 1e3 * dt / args.iters,
        "ms_per_iteration_by_stage": per_iter, "ms_per_iteration_events": events_ms,
        "share_outside_products": 1.0 - per_iter["products"] / events_ms if events_ms > 0 else None,
        "status_flags": flags, "tie_draws": draws,
        "dual_energy_start": e0, "dual_energy_end": energy, "max_violation": max_violation, "sum_violation": sum_violation,
        "generate_seconds": t_generate, "setup_seconds": t_setup,
        "cpu_reference_order_one_core": {
            "rows": int(sample_rows), "iterations": args.cpu_iters, "seconds": cpu_seconds, "it_per_s_on_sample": cpu_sample_rate,
            "it_per_s": cpu_sample_rate * scale, "extrapolated": scale != 1.0,
        },
    }
    out["speedup_vs_cpu"] = out["it_per_s"] / out["cpu_reference_order_one_core"]["it_per_s"]
    solver.close()
    a.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    if args.path != "auto":
        name += "_" + args.path
    with open(os.path.join(args.outdir, f"dga_{name}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
