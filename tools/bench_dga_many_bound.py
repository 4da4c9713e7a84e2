"""The bound cut-off of dual gradient ascent on a list (DeviceDGAMany.set_cutoff, csrc/slp_dga_many.hip, k_dgm_iterate<true, true>):
what the two kernels without it cost against the parent commit, what a check with the bound costs, and what retiring LPs buys.

    python tools/bench_dga_many_bound.py OUTDIR [--parts a,b,c] [--parent-repo DIR] [--counts 1,8,64,256,1024]
                                                [--counts-price 256,1024] [--pruned 1024] [--prune-at 20] [--check-every 10]
                                                [--horizon 200] [--iters 400] [--warmup 20] [--repeats 3] [--seconds 0.3]
                                                [--screen 1500]

Writes one JSON line (stdout and OUTDIR/dga_many_bound.json).  It follows tools/bench_dga_many_stop.py, whose helpers it imports:
the Potts lists of tools/bench_dga_many.py, times between two HIP events on the library's stream (the draw buffers filled
beforehand) except the wall times of part (c), a warm-up, `repeats` measurements that alternate between the variants compared,
the median with every repeat and the spread ((max - min) / median) beside it.

  (a) unchanged  the kernel that is never armed, <false, false>, and the kernel armed with the step alone, <true, false>
                 (tolerance 0 at check_every = 10 on a list screened for exact fixed points, as part (b) of bench_dga_many_stop),
                 instance-iterations/s against the PARENT commit's library on the same box, alternating child processes (one at
                 a time).  --parent-repo names a built checkout of the parent; without it the comparison is null.  The bar, fixed
                 before the run, per N and set: this median >= the parent's median x (1 - the parent's own spread between its
                 repeats); each point is reported as inside, or outside and by how much (`short_of_bar`).
  (b) price      one process: a Potts list never armed, and armed with no tolerance and cut-offs of 1e300 -- a check that cannot
                 fire -- at check_every = 1 and 10.  Recorded: the three rates, the two ratios armed / unarmed and, from
                 time per iteration = 1 / rate, the cost of one check in units of an unarmed iteration,
                 check_every x (unarmed / armed - 1).  An armed `iterate` call reads the records back before it launches; that
                 is part of the price.  No bar.
  (c) buys       `--pruned` Potts LPs.  Half of them get as cut-off the bound an unstopped run shows after `--prune-at`
                 iterations, so they are retired at that check.  Wall time (host clock around `iterate` and a synchronising read,
                 the states created and the draws pushed beforehand) to `--horizon` iterations of: the list without cut-offs; the
                 list with the cut-offs in the kernel; and the loop the feature replaces, `iterate(check_every)`, `report()` and
                 the comparison on the host, which learns which LPs have passed their cut-offs and cannot retire them.
                 Which half matters, because a retired LP keeps its workgroup index and the hardware deals workgroups to its
                 eight XCDs in turn: the kernel form is measured with a random half (seed 0), with the first half of the list and
                 with every second LP -- the pattern that leaves every live LP on four of the eight XCDs.
                 Not measured: a caller that rebuilds a shorter list after every prune.
"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dga_many import fill, potts_list, timed  # noqa: E402
from bench_dga_many_stop import GRIDS, many_state, never_stopping, pick_k, summary  # noqa: E402


# ---------------------------------------------------------------------------------------------------- (a) per library
def rates_unchanged(args):
    """Instance-iterations/s of `iterate(k)` never armed and armed with the step alone, for every count: one measurement each, in
    this process, with the package and the library of whichever checkout --repo names (`set_stop` exists in both)."""
    from pysparselp_amd import _lib

    lib = _lib.lib()
    out = {"off": {}, "step": {}}
    for count in [int(v) for v in args.counts.split(",")]:
        lps, _ = never_stopping(potts_list(count + count // 4 + 2, GRIDS), count, args.screen)
        off, step = many_state(lps), many_state(lps)
        step.set_stop(0.0, 10)
        k = pick_k(lib, off, args.iters, args.warmup, args.seconds)
        step.iterate(args.warmup + 8)
        out["off"][str(count)] = count * k * 1e3 / timed(lib, [off], k)
        out["step"][str(count)] = count * k * 1e3 / timed(lib, [step], k)
        assert not step.stop_state()[1].any()
        off.close()
        step.close()
    return out


def part_unchanged(args):
    def child(repo):
        cmd = [sys.executable, os.path.abspath(__file__), "--child-rates", "--repo", os.path.abspath(repo), "--counts", args.counts,
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--seconds", str(args.seconds), "--screen", str(args.screen)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=900)
        rates = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(f"[unchanged] {os.path.relpath(repo)}: " + "; ".join(f"{name} " + ", ".join(f"N={key} {v:.0f}" for key, v in r.items())
                                                                  for name, r in rates.items()), file=sys.stderr, flush=True)
        return rates

    runs = {"parent": [], "this": []}
    for _ in range(args.repeats):   # alternating, one process at a time
        if args.parent_repo:
            runs["parent"].append(child(args.parent_repo))
        runs["this"].append(child(REPO))
    points = []
    for name, kernel in (("off", "never armed: k_dgm_iterate<false, false>"), ("step", "step alone: k_dgm_iterate<true, false>")):
        for key in runs["this"][0][name]:
            point = {"set": "potts 8..16", "kernel": kernel, "N": int(key),
                     "this_instance_it_per_s": summary([r[name][key] for r in runs["this"]])}
            if runs["parent"]:
                parent = point["parent_instance_it_per_s"] = summary([r[name][key] for r in runs["parent"]])
                point["this_over_parent"] = point["this_instance_it_per_s"]["median"] / parent["median"]
                point["bar"] = 1.0 - parent["spread"]
                point["inside_bar"] = bool(point["this_over_parent"] >= point["bar"])
                point["short_of_bar"] = max(0.0, point["bar"] - point["this_over_parent"])
            points.append(point)
            print(f"[unchanged] {name} N={key}: {point['this_instance_it_per_s']['median']:.0f} instance-it/s, ratio to parent "
                  f"{point.get('this_over_parent')}, bar {point.get('bar')}", file=sys.stderr)
    return {"parent_measured": bool(args.parent_repo), "points": points}


# ---------------------------------------------------------------------------------------------------- (b) the price of a check
def part_price(args, lib):
    points = []
    for count in [int(v) for v in args.counts_price.split(",")]:
        lps = potts_list(count, GRIDS)
        states = {"off": many_state(lps), "every_1": many_state(lps), "every_10": many_state(lps)}
        states["every_1"].set_cutoff(None, 1, 1e300)
        states["every_10"].set_cutoff(None, 10, 1e300)
        k = pick_k(lib, states["off"], args.iters, args.warmup, args.seconds)
        for key in ("every_1", "every_10"):
            states[key].iterate(args.warmup + 8)
        rate = {key: [] for key in states}
        for _ in range(args.repeats):   # alternating
            for key, st in states.items():
                rate[key].append(count * k * 1e3 / timed(lib, [st], k))
        point = {"set": "potts 8..16", "N": count, "iterations_per_measurement": k}
        off = float(np.median(rate["off"]))
        for key, st in states.items():
            point[f"{key}_instance_it_per_s"] = summary(rate[key])
            if key != "off":
                every = int(key.split("_")[1])
                full = st.stop_state_full()
                assert not full[1].any() and np.all(np.isfinite(full[3]))   # every check evaluated a bound, none fired
                point[f"{key}_over_off"] = float(np.median(rate[key])) / off
                point[f"{key}_check_in_iterations"] = every * (off / float(np.median(rate[key])) - 1.0)
            st.close()
        points.append(point)
        print(f"[price] N={count}: unarmed {off:.0f} instance-it/s, check_every 1 x{point['every_1_over_off']:.3f} "
              f"({point['every_1_check_in_iterations']:.3f} it/check), 10 x{point['every_10_over_off']:.3f} "
              f"({point['every_10_check_in_iterations']:.3f} it/check)", file=sys.stderr)
    return {"points": points}


# ---------------------------------------------------------------------------------------------------- (c) what retiring buys
def part_buys(args):
    count, every, horizon = args.pruned, args.check_every, args.horizon
    assert args.prune_at % every == 0 and horizon % every == 0 and horizon > args.prune_at
    lps = potts_list(count, GRIDS)
    st = many_state(lps)
    st.iterate(args.prune_at)
    bound = st.report()[:, 0]
    st.close()
    halves = {"random_half": np.random.RandomState(0).permutation(count) < count // 2, "first_half": np.arange(count) < count // 2,
              "every_second": np.arange(count) % 2 == 0}
    cut = {name: np.where(half, bound, np.inf) for name, half in halves.items()}
    targets = cut["random_half"]   # what the host loop compares with

    def ready(arm):
        st = many_state(lps)
        arm(st)
        fill(st, horizon)
        return st

    def run_kernel(st):
        st.iterate(horizon, refill=False)
        return st.stop_state_full()

    def run_host(st):
        passed = np.zeros(count, dtype=bool)
        for _ in range(horizon // every):
            st.iterate(every, refill=False)
            passed |= st.report()[:, 0] >= targets
        return passed

    variants = {"no_cut_offs": (lambda st: None, lambda st: (st.iterate(horizon, refill=False), st.status())),
                "host_loop_with_report": (lambda st: None, run_host)}
    for name in halves:
        variants["in_the_kernel_" + name] = (lambda st, t=cut[name]: st.set_cutoff(None, every, t), run_kernel)
    wall = {key: [] for key in variants}
    seen = {}
    for rep in range(args.repeats + 1):   # the first round warms up; alternating
        for key, (arm, run) in variants.items():
            st = ready(arm)
            start = time.perf_counter()
            seen[key] = run(st)
            took = time.perf_counter() - start
            st.close()
            if rep:
                wall[key].append(took)
    out = {"set": "potts 8..16", "N": count, "check_every": every, "horizon": horizon, "prune_at": args.prune_at,
           "passed_in_the_host_loop": int(seen["host_loop_with_report"].sum())}
    for key in variants:
        out[f"{key}_wall_s"] = summary(wall[key])
    base = out["no_cut_offs_wall_s"]["median"]
    out["host_loop_over_no_cut_offs"] = out["host_loop_with_report_wall_s"]["median"] / base
    for name in halves:
        full = seen["in_the_kernel_" + name]
        out[f"in_the_kernel_{name}_retired"] = int(full[1].sum())
        out[f"in_the_kernel_{name}_retired_at"] = sorted({int(v) for v in full[0][full[1]]})
        out[f"in_the_kernel_{name}_over_no_cut_offs"] = out[f"in_the_kernel_{name}_wall_s"]["median"] / base
    print(f"[buys] N={count}: no cut-offs {base * 1e3:.1f} ms, host loop x{out['host_loop_over_no_cut_offs']:.3f}, in the kernel "
          + ", ".join(f"{name} x{out[f'in_the_kernel_{name}_over_no_cut_offs']:.3f}" for name in halves), file=sys.stderr)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("outdir", nargs="?")
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--parent-repo", default="")
    p.add_argument("--repo", default="")
    p.add_argument("--counts", default="1,8,64,256,1024")
    p.add_argument("--counts-price", default="256,1024")
    p.add_argument("--pruned", type=int, default=1024)
    p.add_argument("--prune-at", type=int, default=20)
    p.add_argument("--check-every", type=int, default=10)
    p.add_argument("--horizon", type=int, default=200)
    p.add_argument("--iters", type=int, default=400)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seconds", type=float, default=0.3)
    p.add_argument("--screen", type=int, default=1500, help="part a: iterations of the screening run for LPs that reach a fixed point")
    p.add_argument("--child-rates", action="store_true")
    args = p.parse_args()
    assert args.repeats >= 1 and args.iters >= 8

    if args.child_rates:
        if args.repo:   # ahead of this checkout: the package and the library of that one
            sys.path[:0] = [args.repo]
        print(json.dumps(rates_unchanged(args)))
        return
    assert args.outdir, "OUTDIR is missing"
    parts = args.parts.split(",")
    out = {"method": "dual_gradient_ascent_many_cutoff", "box": platform.node(), "device": "AMD Instinct MI355X (gfx950)",
           "iterations": args.iters, "warmup": args.warmup, "repeats": args.repeats}
    if "a" in parts:   # before this process opens the GPU: one process with the device at a time
        out["unchanged_against_parent"] = part_unchanged(args)
    if "b" in parts or "c" in parts:
        from pysparselp_amd import _lib

        lib = _lib.lib()
        if "b" in parts:
            out["price_of_a_check"] = part_price(args, lib)
        if "c" in parts:
            out["what_retiring_buys"] = part_buys(args)
    line = json.dumps(out)
    print(line)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, "dga_many_bound.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
