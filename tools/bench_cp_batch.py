"""Batched Chambolle-Pock (CPBatchState, csrc/slp_cp_batch.hip) measured against the single-instance solver of the same library.

    python tools/bench_cp_batch.py OUTDIR [--workload potts|random|both] [--potts 256] [--rows 100000 --cols 200000 --density 1e-3]
                                          [--batches 1,8,16,32,64,128] [--iters 2000] [--warmup 200] [--repeats 3]

Writes one JSON line (stdout and OUTDIR/cp_batch.json).  Per workload and batch size B, `repeats` times in turn, in one process:
the batched solver (slp_cp_batch_bench: HIP events around `iters` iterations of plain launches, after a warm-up) and the
single-instance solver on instance 0 of the same LP (slp_cp_bench, the same kind of loop) -- in its default format (packed ELL on
Potts) and with the CSR kernels in SEQUENTIAL order, the sums the batch reproduces.  Recorded per point: batched it/s,
instance-iterations/s = B x that, the ratio to the single-instance rates, the spread of the repeats ((max - min) / median), the
bytes one batched iteration must move by the shapes (both CSR orientations once, the vectors B times: 7 n + 4 m doubles per
instance, T and Sigma once) and the resulting bytes/s.

Workload 1: the Potts n x n LP (problems.potts_lp), instance costs = seeded perturbations of the unary costs.
Workload 2: the synthetic random LP (problems.random_lp_on_device) at rows x cols, generated on the device and downloaded;
on it the iteration count per measurement shrinks so that one measurement stays near a second (recorded per point).

`holds_at_64`: on Potts at B = 64 the slowest repeat's instance-iterations/s exceeds the fastest repeat's single-instance
default-format rate -- the ranges of the repeats do not even touch.
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import spread  # noqa: E402


def single_state(c, ineq, b, lb, ub, csr):
    """CPState on one instance: default format, or (csr) the CSR kernels in SEQUENTIAL order."""
    from pysparselp_amd import ORDER_AUTO, ORDER_SEQUENTIAL
    from pysparselp_amd.ChambollePockPPD import CPState

    saved = os.environ.get("SLP_CP_ELL")
    if csr:
        os.environ["SLP_CP_ELL"] = "0"
    try:
        return CPState(c, None, None, ineq, b, lb, ub, None, 1, 1, ORDER_SEQUENTIAL if csr else ORDER_AUTO)
    finally:
        if csr:
            if saved is None:
                del os.environ["SLP_CP_ELL"]
            else:
                os.environ["SLP_CP_ELL"] = saved


def measure(name, c, ineq, b, lb, ub, batches, iters, warmup, repeats, seed, perturb, adapt):
    from pysparselp_amd.ChambollePockPPD import CPBatchState

    indptr, indices, data, m = ineq
    n, nnz = c.size, int(indptr[-1])
    matrix_bytes = 2 * 12 * nnz + 8 * (m + 1) + 8 * (n + 1) + 8 * (n + m)
    default, csr = single_state(c, ineq, b, lb, ub, False), single_state(c, ineq, b, lb, ub, True)
    default.iterate(warmup)
    csr.iterate(warmup)
    points = []
    for batch in batches:
        cs = np.tile(c, (batch, 1))
        cs[1:] += perturb(np.random.RandomState(seed + batch), batch - 1)
        st = CPBatchState(cs, None, None, ineq, b, lb, ub, None, 1, 1)
        st.iterate(warmup)
        k = iters
        if adapt:   # one measurement near a second
            k = int(min(iters, max(20, 1000.0 / st.bench(10)[0])))
        ks = k if not adapt else int(min(iters, max(20, 1000.0 / csr.bench(10)[0])))
        ms_b, ms_d, ms_c = [], [], []
        for _ in range(repeats):   # alternating
            ms_b.append(st.bench(k))
            ms_d.append(default.bench(ks))
            ms_c.append(csr.bench(ks))
        st.close()
        ms_b, ms_d, ms_c = np.array(ms_b), np.array(ms_d), np.array(ms_c)
        it_b, it_d, it_c = 1e3 / ms_b[:, 0], 1e3 / ms_d[:, 0], 1e3 / ms_c[:, 0]
        bytes_it = matrix_bytes + (7 * n + 4 * m) * 8 * batch
        points.append({
            "B": batch, "iterations_per_measurement": k, "single_iterations_per_measurement": ks,
            "batched_it_per_s": float(np.median(it_b)), "batched_it_per_s_repeats": it_b.tolist(), "batched_spread": spread(it_b),
            "instance_it_per_s": float(batch * np.median(it_b)),
            "ms_primal_kernel": float(np.median(ms_b[:, 1])), "ms_dual_kernel": float(np.median(ms_b[:, 2])),
            "single_default_it_per_s": float(np.median(it_d)), "single_default_repeats": it_d.tolist(), "single_default_spread": spread(it_d),
            "single_csr_it_per_s": float(np.median(it_c)), "single_csr_repeats": it_c.tolist(), "single_csr_spread": spread(it_c),
            "ratio_to_single_default": float(batch * np.median(it_b) / np.median(it_d)),
            "ratio_to_single_csr": float(batch * np.median(it_b) / np.median(it_c)),
            "beats_single_default_beyond_spread": bool(batch * it_b.min() > it_d.max()),
            "bytes_per_iteration": int(bytes_it), "bytes_per_s": float(bytes_it * np.median(it_b)),
        })
        print(f"[{name}] B={batch}: {points[-1]['batched_it_per_s']:.0f} it/s batched, {points[-1]['instance_it_per_s']:.0f} instance-it/s, "
              f"single {points[-1]['single_default_it_per_s']:.0f} (default) {points[-1]['single_csr_it_per_s']:.0f} (CSR) it/s", file=sys.stderr)
    default.close()
    csr.close()
    return {"workload": name, "n": int(n), "m": int(m), "nnz": nnz, "matrix_bytes_per_iteration": int(matrix_bytes),
            "vector_bytes_per_instance_iteration": int((7 * n + 4 * m) * 8), "points": points}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--workload", default="both", choices=("potts", "random", "both"))
    p.add_argument("--potts", type=int, default=256)
    p.add_argument("--rows", type=int, default=100000)
    p.add_argument("--cols", type=int, default=200000)
    p.add_argument("--density", type=float, default=1e-3)
    p.add_argument("--batches", default="1,8,16,32,64,128")
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 1
    batches = [int(v) for v in args.batches.split(",")]

    from pysparselp_amd import _lib
    from pysparselp_amd.ChambollePockPPD import one_sided_system
    from pysparselp_amd.problems import potts_lp, random_lp_on_device

    _lib.lib()
    out = {"method": "chambolle_pock_ppd_batch", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats, "workloads": []}
    if args.workload in ("potts", "both"):
        lp, _, pix, _ = potts_lp(args.potts)
        ineq, b = one_sided_system(lp.a_inequalities, lp.b_lower, lp.b_upper)
        npix = pix.size

        def perturb(rs, count, n=lp.nb_variables):
            d = np.zeros((count, n))
            d[:, :npix] = 0.3 * rs.randn(count, npix)   # the unary costs (the pixel variables come first)
            return d

        w = measure(f"potts{args.potts}", lp.costsvector, ineq, b, lp.lower_bounds, lp.upper_bounds, batches, args.iters, args.warmup,
                    args.repeats, args.seed, perturb, adapt=False)
        at64 = [q for q in w["points"] if q["B"] == 64]
        if at64:
            w["holds_at_64"] = at64[0]["beats_single_default_beyond_spread"]
        out["workloads"].append(w)
    if args.workload in ("random", "both"):
        a, _, c, lb, ub, b = random_lp_on_device(args.cols, args.rows, args.density, seed=args.seed)
        host = a.download()
        a.close()
        ineq = _lib.csr_arrays(host) + (host.shape[0],)
        scale = float(np.mean(np.abs(c)))
        w = measure(f"random_{args.rows}x{args.cols}_d{args.density:g}", c, ineq, b, lb, ub, batches, args.iters, args.warmup, args.repeats,
                    args.seed, lambda rs, count: 0.2 * scale * rs.randn(count, c.size), adapt=True)
        pays = [q["B"] for q in w["points"] if q["beats_single_default_beyond_spread"]]
        w["pays_from_B"] = min(pays) if pays else None
        out["workloads"].append(w)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "cp_batch.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
