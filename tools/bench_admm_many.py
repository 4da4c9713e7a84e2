"""ADMM with the projected Gauss-Seidel x-step on a list of LPs (ADMMManyState, csrc/slp_admm_many.hip: one workgroup per LP, whole
iterations inside a launch) measured against the same LPs through the single solver one after another (ADMMState, csrc/slp_admm.hip,
on its own automatic path), in ONE process and ONE run.

    python tools/bench_admm_many.py OUTDIR [--counts 1,8,64,256,1024] [--grids 8,9,...,16] [--warmup 20] [--repeats 3]

Writes one JSON line (stdout and OUTDIR/admm_many.json).  The LPs are Potts LPs of the package's own builder (problems.potts_lp),
grids 8 x 8 to 16 x 16 in rotation, the unary costs of LP k perturbed with seed k (distinct costs).  Per N one row: the list
form's instance-iterations per second (N x iterations of the list / time), the partner's (the N single solvers iterated one
after another, the same number of iterations each), their ratio, and as the ceiling a shared matrix gives: the batched solver
(ADMMBatchState) on the 12 x 12 LP with N costs.  Every rate is a pair of HIP events (slp_timer_start / _stop) around the timed
iterations, after a warm-up; `repeats` measurements alternate between the list form, the partner and the batch; the median is
reported with all repeats.  Condition `many_above_single_at_256`: at N = 256 the list form's slowest repeat is above the
partner's fastest.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def potts_list(count, grids):
    """`count` 8-tuples (c, a_eq, beq, a_ineq, b_lower, b_upper, lb, ub) as lp_admm takes them."""
    from pysparselp_amd.problems import potts_lp

    base = {}
    out = []
    for k in range(count):
        size = grids[k % len(grids)]
        if size not in base:
            lp, _, pix, _ = potts_lp(size)
            base[size] = (lp, pix.size)
        lp, npix = base[size]
        c = np.array(lp.costsvector, dtype=np.float64)
        c[:npix] += 0.3 * np.random.RandomState(1000 + k).randn(npix)   # the unary costs come first
        has_eq = lp.a_equalities.shape[0] > 0
        out.append((c, lp.a_equalities if has_eq else None, lp.b_equalities if has_eq else None, lp.a_inequalities, lp.b_lower,
                    lp.b_upper, lp.lower_bounds, lp.upper_bounds))
    return out


def timed(lib, states, k):
    """Milliseconds for `k` iterations of every state, one state after another, between two HIP events."""
    from pysparselp_amd import _lib

    ms = np.zeros(1)
    _lib.check(lib.slp_timer_start())
    for st in states:
        st.iterate(k)
    _lib.check(lib.slp_timer_stop(_lib.ptr(ms)))
    return float(ms[0])


def iterations_for(lib, states, target_ms, cap):
    return int(min(cap, max(5, target_ms / max(timed(lib, states, 5) / 5, 1e-6))))


def measure(count, grids, warmup, repeats, target_ms):
    from pysparselp_amd import _lib
    from pysparselp_amd.ADMM import ADMMBatchState, ADMMManyState, ADMMState, _admm_many_problem

    lib = _lib.lib()
    problems = potts_list(count, grids)
    many = ADMMManyState([_admm_many_problem(k, p) for k, p in enumerate(problems)])
    singles = [ADMMState.from_lp(*p, None, 2, 3) for p in problems]
    # the ceiling of a shared matrix: N costs over the LP of the middle grid
    mid = potts_list(len(grids), grids)[len(grids) // 2]
    costs = np.tile(mid[0], (count, 1))
    costs[1:] += 0.01 * np.random.RandomState(5).randn(count - 1, costs.shape[1])
    batch = ADMMBatchState(costs, *mid[1:])
    sets = {"many": [many], "single": singles, "batch": [batch]}
    for states in sets.values():
        for st in states:
            st.iterate(warmup)
    k = {name: iterations_for(lib, states, target_ms, 2000) for name, states in sets.items()}
    ms = {name: [] for name in sets}
    for _ in range(repeats):   # alternating
        for name, states in sets.items():
            ms[name].append(timed(lib, states, k[name]))
    rate = {name: count * k[name] * 1e3 / np.array(v) for name, v in ms.items()}   # instance-iterations per second
    forms = sorted({many.form(j) for j in range(count)})
    point = {"N": count, "n_min": int(many.n.min()), "n_max": int(many.n.max()), "unknowns_max": int(many.N.max()), "rows_max": int(many.m.max()),
             "levels_min": min(many.num_levels(j) for j in range(count)), "levels_max": max(many.num_levels(j) for j in range(count)),
             "forms": forms, "iterations_per_launch_cap": {f: many.kmax(f) for f in forms}, "batch_form": batch.form(),
             "iterations_per_measurement": k,
             "many_instance_it_per_s": float(np.median(rate["many"])), "many_repeats": rate["many"].tolist(),
             "single_instance_it_per_s": float(np.median(rate["single"])), "single_repeats": rate["single"].tolist(),
             "batch_shared_matrix_instance_it_per_s": float(np.median(rate["batch"])), "batch_repeats": rate["batch"].tolist(),
             "ratio_to_single": float(np.median(rate["many"]) / np.median(rate["single"])),
             "many_slowest_above_single_fastest": bool(rate["many"].min() > rate["single"].max())}
    for states in sets.values():
        for st in states:
            st.close()
    print(f"N={count}: list {point['many_instance_it_per_s']:.0f}, one after another {point['single_instance_it_per_s']:.0f}, shared matrix "
          f"{point['batch_shared_matrix_instance_it_per_s']:.0f} instance-it/s; x {point['ratio_to_single']:.2f}", file=sys.stderr)
    return point


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--counts", default="1,8,64,256,1024")
    p.add_argument("--grids", default="8,9,10,11,12,13,14,15,16")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--target-ms", type=float, default=400.0)
    args = p.parse_args()
    assert args.repeats >= 1
    grids = [int(v) for v in args.grids.split(",")]
    out = {"method": "admm_many", "device": "AMD Instinct MI355X (gfx950)", "grids": grids, "warmup": args.warmup, "repeats": args.repeats,
           "points": []}
    for count in (int(v) for v in args.counts.split(",")):
        out["points"].append(measure(count, grids, args.warmup, args.repeats, args.target_ms))
    at256 = [q for q in out["points"] if q["N"] == 256]
    if at256:
        out["many_above_single_at_256"] = bool(at256[0]["many_slowest_above_single_fastest"])
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "admm_many.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
