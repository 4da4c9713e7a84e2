"""The certificate on the two single ADMM solvers (slp_admm_set_stop_gap / slp_admm_cg_set_stop_gap; csrc/slp_admm.hip
k_admm_gap_dual / k_admm_gap_cols / k_admm_gap_rows, csrc/slp_admm_cg.hip k_cg_gap_dual / k_cg_gap_cols / k_cg_gap_rows, the fold of
csrc/slp_gap_fold.h): that the unarmed solver is the parent's, what a check costs, and the time to a certified gap on config 3.

    python tools/bench_admm_gap.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--repeats 3] [--potts 256] [--c3-iters 60]
                                          [--potts-iters 2000] [--warmup 20] [--max-iters 5000]

Writes one JSON line (stdout and OUTDIR/admm_gap.json).  The method is tools/bench_cp_gap.py's: HIP events on the library's
stream (slp_timer_start / _stop) around iterate(k), a warm-up, `--repeats` repeats alternating between the variants, medians, every
repeat and the spread (max - min) / median in the file.  Workloads: config 3 (problems.random_lp_on_device, 1e6 variables x 2e6
rows at 1e-3, DeviceADMM at reuse level 4) and Potts-256 (ADMMState, the Gauss-Seidel x-step on the explicit M).

  (a) unarmed against the parent commit: iterations/s of a state that was never armed, alternating child processes of the two
      checkouts (--parent-repo: a built checkout of the parent), one at a time.  The bar, fixed before the run: this median >=
      the parent's median x (1 - the parent's own spread).
  (b) the price of a check: one state, disarmed / armed at check_every = 1 / armed at check_every = 10 in turn, tolerances of 0
      (never met: the tool asserts that nothing stopped); per check (armed - unarmed) / checks, in microseconds and in iterations
      of the unarmed state.  No bar.
  (c) time to a certified 1e-2 / 1e-2 on config 3 at check_every = 10 within --max-iters iterations: wall seconds, iterations,
      and the certificate it ended on.  No bar.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = (1_000_000, 2_000_000, 1e-3)   # bench.py CONFIGS["c3"]: variables, rows, density


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return float((v.max() - v.min()) / np.median(v)) if v.size > 1 else 0.0


def summary(values):
    return {"median": float(np.median(values)), "repeats": [float(v) for v in values], "spread": spread(values)}


def make_state(workload, potts):
    """An unarmed state of the workload and what to close afterwards; uses nothing the parent commit does not have."""
    if workload == "c3":
        from pysparselp_amd.admm_cg import DeviceADMM
        from pysparselp_amd.problems import random_lp_on_device

        a, _, c, lb, ub, b = random_lp_on_device(*C3, seed=0)
        return DeviceADMM(a, b, c, lb, ub, reuse=4), [a]
    from pysparselp_amd.ADMM import ADMMState
    from pysparselp_amd.problems import potts_lp

    lp = potts_lp(potts)[0]
    a_eq = lp.a_equalities if lp.a_equalities is not None and lp.a_equalities.shape[0] else None
    return ADMMState.from_lp(lp.costsvector, a_eq, lp.b_equalities if a_eq is not None else None, lp.a_inequalities, lp.b_lower,
                             lp.b_upper, lp.lower_bounds, lp.upper_bounds, None, 2, 3), []


def timed(lib, st, k):
    """(milliseconds between two HIP events, wall seconds) of st.iterate(k); ends synchronised."""
    from pysparselp_amd import _lib

    ms = np.zeros(1)
    start = time.perf_counter()
    _lib.check(lib.slp_timer_start())
    st.iterate(k)
    _lib.check(lib.slp_timer_stop(_lib.ptr(ms)))
    return float(ms[0]), time.perf_counter() - start


def iterations_of(args, workload):
    return args.c3_iters if workload == "c3" else args.potts_iters


# ---------------------------------------------------------------------------------------------------- (a) against the parent
def child_rate(args):
    sys.path.insert(0, os.path.abspath(args.repo))
    from pysparselp_amd import _lib

    lib = _lib.lib()
    st, owned = make_state(args.child_rate, args.potts)
    k = iterations_of(args, args.child_rate)
    st.iterate(args.warmup)
    ms, _ = timed(lib, st, k)
    st.close()
    for o in owned:
        o.close()
    print(json.dumps({"it_per_s": k * 1e3 / ms}))


def part_unchanged(args, workloads):
    def child(where, workload):
        cmd = [sys.executable, os.path.abspath(__file__), "--child-rate", workload, "--repo", os.path.abspath(where), "--potts", str(args.potts),
               "--c3-iters", str(args.c3_iters), "--potts-iters", str(args.potts_iters), "--warmup", str(args.warmup), "unused"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=600)
        return json.loads(done.stdout.decode().strip().splitlines()[-1])["it_per_s"]

    points = []
    for workload in workloads:
        runs = {"parent": [], "this": []}
        for _ in range(args.repeats):   # alternating, one process at a time
            if args.parent_repo:
                runs["parent"].append(child(args.parent_repo, workload))
            runs["this"].append(child(REPO, workload))
        point = {"workload": workload, "this_it_per_s": summary(runs["this"])}
        if runs["parent"]:
            point["parent_it_per_s"] = summary(runs["parent"])
            point["this_over_parent"] = point["this_it_per_s"]["median"] / point["parent_it_per_s"]["median"]
            point["bar"] = 1.0 - point["parent_it_per_s"]["spread"]
            point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
        points.append(point)
        print(f"[unarmed] {workload}: {point['this_it_per_s']['median']:.1f} it/s, ratio to parent {point.get('this_over_parent')}, "
              f"bar {point.get('bar')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points}


# ---------------------------------------------------------------------------------------------------- (b) the price of a check
def part_price(args, lib, st, workload):
    k = iterations_of(args, workload)
    k -= k % 10
    variants = (("unarmed", None), ("every1", 1), ("every10", 10))
    runs = {name: {"ms": [], "wall_s": [], "checks": 0} for name, _ in variants}
    st.iterate(args.warmup)
    for every in (1, 10):   # the certificate's buffers and first launches are not measured
        st.set_stop_gap(0.0, 0.0, every)
        st.iterate(10)
    for _ in range(args.repeats):   # alternating
        for name, every in variants:
            if every is None:
                st.set_stop_gap(None, 0.0)
            else:
                st.set_stop_gap(0.0, 0.0, every)
            before = st.gap_state()[0]
            ms, wall = timed(lib, st, k)
            after, stopped = st.gap_state()[:2]
            assert after == before + k and not stopped, (name, before, after, stopped)
            runs[name]["ms"].append(ms)
            runs[name]["wall_s"].append(wall)
            runs[name]["checks"] = 0 if every is None else after // every - before // every
    out = {"workload": workload, "iterations": k}
    base = float(np.median(runs["unarmed"]["ms"]))
    for name, _ in variants:
        r = runs[name]
        out[name] = {"ms": summary(r["ms"]), "wall_s": summary(r["wall_s"]), "checks": int(r["checks"])}
        if r["checks"]:
            per_check = (float(np.median(r["ms"])) - base) / r["checks"]
            out[name]["ms_per_check"] = per_check
            out[name]["us_per_check"] = per_check * 1e3
            out[name]["iterations_per_check"] = per_check / (base / k)
            wall = (float(np.median(r["wall_s"])) - float(np.median(runs["unarmed"]["wall_s"]))) / r["checks"]
            out[name]["wall_iterations_per_check"] = wall / (float(np.median(runs["unarmed"]["wall_s"])) / k)
    out["ms_per_iteration_unarmed"] = base / k
    st.set_stop_gap(None, 0.0)
    print(f"[price] {workload}: {out['every1'].get('iterations_per_check')} / {out['every10'].get('iterations_per_check')} iterations "
          "per check at check_every = 1 / 10", file=sys.stderr)
    return out


# ---------------------------------------------------------------------------------------------------- (c) time to a gap
def part_time_to_gap(args, lib):
    st, owned = make_state("c3", args.potts)   # a fresh matrix: DeviceADMM normalises the rows of its matrix in place
    st.set_stop_gap(1e-2, 1e-2, 10)
    lib.slp_synchronize()
    start = time.perf_counter()
    while True:
        st.iterate(500)
        iterations, stopped, primal, bound, violation = st.gap_state()
        if stopped or iterations >= args.max_iters:
            break
    wall = time.perf_counter() - start
    st.close()
    for o in owned:
        o.close()
    gap = abs(primal - bound) / (1.0 + abs(primal) + abs(bound))
    print(f"[time to gap] config 3: stopped={stopped} after {iterations} iterations, {wall:.2f} s, relative gap {gap}", file=sys.stderr)
    return {"workload": "c3", "tol_gap": 1e-2, "tol_feas": 1e-2, "check_every": 10, "max_iters": args.max_iters, "stopped": bool(stopped),
            "iterations": int(iterations), "wall_s": wall, "primal": primal, "lower_bound": bound, "violation": violation,
            "relative_gap": gap}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--workloads", default="potts,c3")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--potts", type=int, default=256)
    p.add_argument("--c3-iters", type=int, default=60)
    p.add_argument("--potts-iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--max-iters", type=int, default=5000)
    p.add_argument("--child-rate", default="")
    p.add_argument("--repo", default=REPO)
    args = p.parse_args()
    if args.child_rate:
        return child_rate(args)
    sys.path.insert(0, REPO)
    from pysparselp_amd import _lib

    parts, workloads = args.parts.split(","), args.workloads.split(",")
    out = {"tool": "bench_admm_gap", "potts": args.potts, "c3": list(C3), "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process at a time
        out["unarmed_against_parent"] = part_unchanged(args, workloads)
    lib = _lib.lib()
    if "b" in parts:
        out["price_of_a_check"] = []
    for workload in workloads:
        if "b" in parts:
            st, owned = make_state(workload, args.potts)
            out["price_of_a_check"].append(part_price(args, lib, st, workload))
            st.close()
            for o in owned:
                o.close()
        if "c" in parts and workload == "c3":
            out["time_to_gap"] = part_time_to_gap(args, lib)
    line = json.dumps(out)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "admm_gap.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
