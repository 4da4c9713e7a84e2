"""Batched dual gradient ascent (DeviceDGABatch, csrc/slp_dga_batch.hip) measured against the single-instance solver of the same
library (DeviceDGA, csrc/slp_dga.hip), in ONE process and ONE run.

    python tools/bench_dga_batch.py OUTDIR [--potts 256,50] [--batches 1,8,32,64,256] [--iters 2000] [--warmup 50] [--repeats 3]

Writes one JSON line (stdout and OUTDIR/dga_batch.json).  Per Potts n x n LP (problems.potts_lp; instance costs = seeded
perturbations of the unary costs, instance 0 the LP's own): the single-instance iterations per second on instance 0, on every
search path its size allows, and per batch size B and path (the general path with each of its two sorts) the batched iterations per second, instance-iterations/s = B x that,
and their ratio to the single solver's best path.  Every rate is a pair of HIP events (slp_timer_start / _stop) around the timed
iterations of plain launches, after a warm-up, the draw buffer filled beforehand so that nothing is read back in between;
`repeats` measurements alternate between batched and single, the median is reported with the spread (max - min) / median.  The
iteration count of a measurement shrinks so that it stays near a second.  A further run of each point with the stage timer on
(slp_batch_dga_timing_read) gives the per-stage split in milliseconds per iteration.  Reads nothing outside the repository.
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from _bench_util import spread, timed_between_events  # noqa: E402

FUSED_MAX = 8192


def timed(lib, state, k):
    """Milliseconds per iteration of `k` iterations between two HIP events; the draws are pushed first."""
    return timed_between_events(lib, [state], k, lambda st, k: st.push_random(np.random.RandomState(17).random_sample(2 * k + 2))) / k


def stages(state, k):
    state.push_random(np.random.RandomState(18).random_sample(2 * k + 2))
    state.timing(True)
    state.iterate(k, refill=False)
    state.timing(False)
    return {name: v / k for name, v in state.timing_read().items()}


def iterations_near_a_second(lib, state, cap):
    return int(min(cap, max(10, 1000.0 / timed(lib, state, 5))))


def measure(size, batches, iters, warmup, repeats, seed):
    from pysparselp_amd import _lib
    from pysparselp_amd.DualGradientAscent import DeviceDGA, DeviceDGABatch
    from pysparselp_amd.device import DeviceMatrix
    from pysparselp_amd.problems import potts_lp

    lib = _lib.lib()
    lp, _, pix, _ = potts_lp(size)
    assert lp.b_lower is None or np.max(lp.b_lower) == -np.inf
    a_eq, a_ineq = lp.a_equalities, lp.a_inequalities
    m_eq = a_eq.shape[0]
    c, lb, ub = lp.costsvector, lp.lower_bounds, lp.upper_bounds
    n, npix = c.size, pix.size
    b = np.concatenate((lp.b_equalities if m_eq else np.zeros(0), lp.b_upper))
    mat = DeviceMatrix.from_blocks(a_eq if m_eq else None, a_ineq, n)
    m = mat.shape[0]
    paths = ("fused", "general") if n <= FUSED_MAX else ("general",)
    batch_paths = paths[:-1] + ("general-segmented", "general-global")   # the general search with either of its sorts

    def start():
        rs = np.random.RandomState(0)
        return np.concatenate((-rs.rand(m_eq), np.abs(rs.rand(m - m_eq)))), rs

    singles = {}
    for path in paths:
        y0, rs = start()
        st = DeviceDGA(mat, b, c, lb, ub, y0, m_eq=m_eq, draws=rs.random_sample, path=path)
        st.iterate(warmup)
        singles[path] = (st, iterations_near_a_second(lib, st, iters))
    single_ms = {path: [] for path in paths}
    points = []
    for batch in batches:
        costs = np.tile(c, (batch, 1))
        costs[1:, :npix] += 0.3 * np.random.RandomState(seed + batch).randn(batch - 1, npix)   # the unary costs come first
        for path in batch_paths:
            y0, rs = start()
            os.environ.pop("SLP_DGA_BATCH_SORT", None)
            if "-" in path:
                os.environ["SLP_DGA_BATCH_SORT"] = path.partition("-")[2]
            st = DeviceDGABatch(mat, b, costs, lb, ub, y0, m_eq=m_eq, draws=rs.random_sample, path=path.partition("-")[0])
            os.environ.pop("SLP_DGA_BATCH_SORT", None)
            st.iterate(warmup)
            k = iterations_near_a_second(lib, st, iters)
            ms = []
            for _ in range(repeats):   # alternating with the single solver
                ms.append(timed(lib, st, k))
                for sp in paths:
                    single_ms[sp].append(timed(lib, singles[sp][0], singles[sp][1]))
            split = stages(st, max(5, k // 4))
            flags, draws, _, done = st.status()
            assert not np.any(flags), flags
            st.close()
            rate = 1e3 / np.array(ms)
            points.append({"B": batch, "path": path, "iterations_per_measurement": k, "iterations_done": done,
                           "batched_it_per_s": float(np.median(rate)), "batched_it_per_s_repeats": rate.tolist(), "spread": spread(rate),
                           "instance_it_per_s": float(batch * np.median(rate)), "instance_it_per_s_slowest": float(batch * rate.min()),
                           "ms_per_iteration_by_stage": split, "tie_draws_max": int(draws.max())})
            print(f"[potts{size}] B={batch} {path}: {points[-1]['batched_it_per_s']:.0f} it/s, {points[-1]['instance_it_per_s']:.0f} "
                  f"instance-it/s", file=sys.stderr)
    single = {}
    for path in paths:
        rate = 1e3 / np.array(single_ms[path])
        single[path] = {"it_per_s": float(np.median(rate)), "fastest": float(rate.max()), "spread": spread(rate),
                        "measurements": int(rate.size), "iterations_per_measurement": singles[path][1]}
        singles[path][0].close()
    best = max(single[p]["it_per_s"] for p in paths)
    best_fastest = max(single[p]["fastest"] for p in paths)
    for q in points:
        q["ratio_to_single"] = q["instance_it_per_s"] / best
        q["beats_single_beyond_spread"] = bool(q["instance_it_per_s_slowest"] > best_fastest)
    mat.close()
    return {"workload": f"potts{size}", "n": int(n), "m": int(m), "m_eq": int(m_eq), "paths": list(batch_paths), "single": single,
            "single_best_it_per_s": best, "points": points}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--potts", default="256,50")
    p.add_argument("--batches", default="1,8,32,64,256")
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 10
    batches = [int(v) for v in args.batches.split(",")]
    out = {"method": "dual_gradient_ascent_batch", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations_cap": args.iters, "warmup": args.warmup, "repeats": args.repeats, "workloads": []}
    for size in (int(v) for v in args.potts.split(",")):
        w = measure(size, batches, args.iters, args.warmup, args.repeats, args.seed)
        at64 = [q for q in w["points"] if q["B"] == 64]
        if at64:
            w["batched_above_single_at_64"] = bool(any(q["beats_single_beyond_spread"] for q in at64))
        out["workloads"].append(w)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "dga_batch.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
